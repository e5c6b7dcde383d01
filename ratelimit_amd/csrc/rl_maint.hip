// rl_maint.hip — the engine side of the synchronous maintenance calls (export,
// import, lookup, hot keys, scan, forget, the three resizes), each serial and
// ordered after all submitted batches; what they share is the helpers below
// (DESIGN.md section 27).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ratelimit_hip.h"
#include "rl_device.h"
#include "rl_kernels.h"
#include "rl_log_geom.h"
#include "rl_stem_list.h"
#include "rl_engine.h"
#include "rl_engine_int.h"

using namespace rl;

namespace {

// How a call begins its device work: pending request batches complete (a call
// with cheap returns before this has settled them already), the device is set,
// the serial stream waits for every batch. floor: also read the sweep floor.
int call_begin(Engine* c, hipStream_t* st, int64_t* floor = nullptr) {
  RQ_SETTLE(c);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  *st = c->stream;
  HIPCHK(c, after_batches(c, *st));
  if (floor) {
    HIPCHK(c, hipMemcpyAsync(floor, c->s[0].time_floor, 8, hipMemcpyDeviceToHost, *st));
    HIPCHK(c, hipStreamSynchronize(*st));
  }
  return RL_OK;
}

// rl_stem_list.h's check in a call's words: "gpu: <list> offsets must start at
// 0", "gpu: <entry> <i>: <fault>", `over` for a total over the cap.
template <bool AllowEmpty, uint32_t MaxLen>
int stems_check(Engine* c, uint32_t n, const uint32_t* off, uint64_t cap, const char* list, const char* entry,
                const char* fault, const char* over) {
  const rlstem::Bad b = rlstem::check<AllowEmpty, MaxLen>(n, off, cap);
  if (b.what == rlstem::START) return set_err(c, RL_E_INVALID, std::string("gpu: ") + list + " offsets must start at 0");
  if (b.what == rlstem::ENTRY)
    return set_err(c, RL_E_INVALID, std::string("gpu: ") + entry + " " + std::to_string(b.i) + ": " + fault);
  return b.what == rlstem::TOTAL ? set_err(c, RL_E_CAPACITY, over) : RL_OK;
}

// o's seven per-record arrays through get(&array, nrec): DevBufs::get or scan's grown staging.
template <typename Get>
hipError_t records_arrays(ExportDev& o, size_t nrec, Get get) {
  hipError_t e = get(&o.off, nrec);
  if (e == hipSuccess) e = get(&o.unit, nrec);
  if (e == hipSuccess) e = get(&o.flags, nrec);
  if (e == hipSuccess) e = get(&o.ws, nrec);
  if (e == hipSuccess) e = get(&o.count, nrec);
  if (e == hipSuccess) e = get(&o.expire, nrec);
  if (e == hipSuccess) e = get(&o.lc, nrec);
  return e;
}

// nrec records / nb stem bytes of o to out at record r0 / byte b0 (the end offset is the caller's).
hipError_t records_to_host(const ExportDev& o, uint64_t nrec, uint64_t nb, rl_records* out, uint64_t r0, uint64_t b0,
                           hipStream_t st) {
  hipError_t e = hipMemcpyAsync(out->stem_bytes + b0, o.stem, nb, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out->stem_off + r0, o.off, nrec * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out->unit + r0, o.unit, nrec, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out->flags + r0, o.flags, nrec, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out->ws + r0, o.ws, nrec * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out->count + r0, o.count, nrec * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out->expire + r0, o.expire, nrec * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out->lc + r0, o.lc, nrec * 4, hipMemcpyDeviceToHost, st);
  return e;
}

// n prefixes into buffers of RL_FORGET_PREFIX_BYTES / RL_FORGET_PREFIX_MAX + 1; zero: bytes cleared first.
hipError_t prefix_upload(uint8_t* d_pfx, uint32_t* d_poff, const uint8_t* bytes, const uint32_t* off, uint32_t n,
                         bool zero, hipStream_t st) {
  hipError_t e = zero ? hipMemsetAsync(d_pfx, 0, RL_FORGET_PREFIX_BYTES, st) : hipSuccess;
  if (!n) return e;
  if (e == hipSuccess) e = hipMemcpyAsync(d_pfx, bytes, off[n], hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_poff, off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st);
  return e;
}

// device staging that lives with the engine: at least `need` elements, never shrunk
template <typename T>
hipError_t scan_grow(T** p, size_t* cap, size_t need) {
  if (need <= *cap) return hipSuccess;
  const size_t want = std::max(need, *cap + *cap / 2);
  T* q = nullptr;
  const hipError_t e = dalloc(&q, want);
  if (e != hipSuccess) return e;
  if (*p) (void)hipFree(*p);
  *p = q;
  *cap = want;
  return hipSuccess;
}

// A placement or commit that fails: the plan is emptied, so nothing is held.
template <typename Plan>
int plan_fail(Engine* c, Plan* p, int code, const std::string& msg) {
  eng_plan_abort(c, p);
  return set_err(c, code, msg);
}

// A commit's end: the plan now holds the old memory, which goes; its info stays.
template <typename Plan>
void plan_finish(Engine* c, Plan* p) {
  const auto info = p->info;
  eng_plan_abort(c, p);
  p->info = info;
}

}  // namespace

namespace rl {

bool records_check(const rl_records* r, bool every_column) {
  if (!r->stem_off || (r->stem_cap && !r->stem_bytes)) return false;
  if (!every_column && !r->n) return true;
  return r->unit && r->flags && r->ws && r->count && r->expire && r->lc;
}

int eng_export_range(Engine* c, uint64_t s0, uint64_t s1, rl_records* out, rl_export_info* info) {
  if (!c || !info) return set_err(c, RL_E_INVALID, "gpu: null argument");
  RQ_SETTLE(c);
  if (out && !records_check(out)) return set_err(c, RL_E_INVALID, "gpu: null rl_records array");
  hipStream_t st;
  if (const int rc = call_begin(c, &st)) return rc;
  s1 = std::min<uint64_t>(s1, c->nslots);
  s0 = std::min(s0, s1);
  *info = rl_export_info{};
  info->shard_slots = c->nslots;
  HIPCHK(c, hipMemcpyAsync(&info->time_floor, c->s[0].time_floor, 8, hipMemcpyDeviceToHost, st));
  DevBufs mem;
  uint32_t* cnt = nullptr;
  unsigned long long* tot = nullptr;  // [0..3] the range's sums, [4] the write cursor
  unsigned long long h_tot[5] = {};
  if (s1 > s0) {
    HIPCHK(c, mem.get(&cnt, s1 - s0));
    HIPCHK(c, mem.get(&tot, 5));
    HIPCHK(c, hipMemsetAsync(tot, 0, 40, st));
    launch_export_count(table_view(c), s0, s1, cnt, tot, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_tot, tot, 40, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  const uint64_t nrec = h_tot[0], nb = h_tot[1];
  info->records = nrec;
  info->stem_bytes = nb;
  info->keys = h_tot[2];
  info->chains_lost = h_tot[3];
  if (!out) return RL_OK;
  // (stem_off is 32-bit per call: a range holding 4 GiB of stems goes out in smaller ranges)
  if (nrec > out->n || nb > out->stem_cap || nb > 0xFFFFFFFFull)
    return set_err(c, RL_E_CAPACITY,
                   "gpu: export range holds " + std::to_string(nrec) + " records / " + std::to_string(nb) +
                       " stem bytes: larger than rl_records (or 4 GiB of stems: export smaller ranges)");
  out->n = (uint32_t)nrec;
  out->stem_off[0] = 0;
  if (!nrec) return RL_OK;
  ExportDev o{};
  HIPCHK(c, mem.get(&o.stem, nb));
  HIPCHK(c, records_arrays(o, nrec, [&](auto** p, size_t k) { return mem.get(p, k); }));
  launch_export_write(table_view(c), s0, s1, cnt, tot + 4, o, st);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, records_to_host(o, nrec, nb, out, 0, 0, st));
  HIPCHK(c, hipMemcpyAsync(h_tot + 4, tot + 4, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  out->stem_off[nrec] = (uint32_t)nb;
  if (h_tot[4] != ((nrec << 32) | nb)) return set_err(c, RL_E_INTERNAL, "gpu: export wrote other than it counted");
  return RL_OK;
}

int eng_hot_check(Engine* c, const rl_hot_query* q) {
  if (!c || !q) return set_err(c, RL_E_INVALID, "gpu: null argument");
  if (q->flags & ~RL_HOT_BLOCKED) return set_err(c, RL_E_INVALID, "gpu: rl_hot_keys: unknown flags");
  if (q->unit_mask & ~rlhot::UNIT_BITS) return set_err(c, RL_E_INVALID, "gpu: rl_hot_keys: unit_mask bit outside 1..4");
  if ((q->flags & RL_HOT_BLOCKED) && !c->cfg.local_cache_enabled)
    return set_err(c, RL_E_INVALID, "gpu: rl_hot_keys: RL_HOT_BLOCKED on a ctx without local cache");
  if (q->k > c->cfg.max_batch) return set_err(c, RL_E_CAPACITY, "gpu: rl_hot_keys: k exceeds configured max_batch");
  if (q->now < 0 || q->now > (int64_t)NOW_MAX) return set_err(c, RL_E_TIME, "gpu: now out of range");
  return RL_OK;
}

int eng_hot_keys(Engine* c, const rl_hot_query* q, HotAnswer* ans, rl_hot_info* info) {
  if (!c || !q || !ans || !info) return set_err(c, RL_E_INVALID, "gpu: null argument");
  if (const int rc = eng_hot_check(c, q)) return rc;
  hipStream_t st;
  int64_t floor = 0;
  if (const int rc = call_begin(c, &st, &floor)) return rc;
  if (q->now < floor) return set_err(c, RL_E_TIME, "gpu: now below the sweep floor");
  const uint32_t k = q->k;
  const uint64_t range = std::min<uint64_t>(c->hot_range, c->nslots);
  const uint64_t pool_cap = k ? range + 2ull * k : 0;  // (< 2^32: range <= 2^22, k <= max_batch <= 2^23)
  const rlhot::Query dq{(uint32_t)q->now, q->min_count, q->unit_mask, q->flags};
  DevBufs mem;
  HotState* hs = nullptr;
  unsigned long long* pool = nullptr;
  HIPCHK(c, mem.get(&hs, 1));
  if (k) HIPCHK(c, mem.get(&pool, pool_cap));
  HIPCHK(c, hipMemsetAsync(hs, 0, sizeof(HotState), st));
  const TableDev t = table_view(c);
  // The ranges start small and double up to `range`: the first cut then runs
  // on a pool of a few K entries, not on every match of 2^22 slots (one
  // workgroup selects), and with its threshold the later ranges add little.
  for (uint64_t s0 = 0, r = std::min<uint64_t>(range, 4096); s0 < c->nslots; r = std::min(2 * r, range)) {
    const uint64_t s1 = std::min(s0 + r, c->nslots);
    launch_hot_scan(t, s0, s1, dq, k, hs, pool, (uint32_t)pool_cap, st);
    if (k) launch_hot_select(hs, pool, (uint32_t)pool_cap, k, 2 * k, st);
    s0 = s1;
  }
  if (k) {
    launch_hot_select(hs, pool, (uint32_t)pool_cap, k, k, st);
    launch_hot_size(t, hs, pool, (uint32_t)pool_cap, k, st);
  }
  HIPCHK(c, hipGetLastError());
  HotState h{};
  HIPCHK(c, hipMemcpyAsync(&h, hs, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (h.err || h.pool_n > k) return set_err(c, RL_E_INTERNAL, "gpu: rl_hot_keys: the candidate pool overflowed");
  *info = rl_hot_info{};
  info->slots = c->nslots;
  info->matched = h.matched;
  info->hits = h.hits;
  info->time_floor = floor;
  const uint32_t n = h.pool_n;
  const uint64_t nb = h.stem_bytes;
  *ans = HotAnswer{};
  if (!n) return RL_OK;
  HotOutDev o{};
  o.stem_cap = nb;
  HIPCHK(c, mem.get(&o.stem, nb));
  HIPCHK(c, mem.get(&o.off, n));
  HIPCHK(c, mem.get(&o.len, n));
  HIPCHK(c, mem.get(&o.unit, n));
  HIPCHK(c, mem.get(&o.ws, n));
  HIPCHK(c, mem.get(&o.count, n));
  HIPCHK(c, mem.get(&o.expire, n));
  HIPCHK(c, mem.get(&o.lc, n));
  launch_hot_gather(t, hs, pool, n, o, st);
  HIPCHK(c, hipGetLastError());
  ans->stem.resize(nb);
  ans->unit.resize(n);
  for (std::vector<uint32_t>* v : {&ans->off, &ans->len, &ans->ws, &ans->count, &ans->expire, &ans->lc}) v->resize(n);
  HIPCHK(c, hipMemcpyAsync(ans->stem.data(), o.stem, nb, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(ans->off.data(), o.off, n * 4ull, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(ans->len.data(), o.len, n * 4ull, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(ans->unit.data(), o.unit, n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(ans->ws.data(), o.ws, n * 4ull, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(ans->count.data(), o.count, n * 4ull, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(ans->expire.data(), o.expire, n * 4ull, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(ans->lc.data(), o.lc, n * 4ull, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(&h, hs, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (h.err || h.cursor != nb) return set_err(c, RL_E_INTERNAL, "gpu: rl_hot_keys gathered other than it sized");
  return RL_OK;
}

int eng_scan_check(Engine* c, const rl_scan_query* q, const rl_records* out) {
  if (!c || !q) return set_err(c, RL_E_INVALID, "gpu: null argument");
  if (q->flags & ~(RL_SCAN_NEWEST | RL_SCAN_LIVE)) return set_err(c, RL_E_INVALID, "gpu: rl_scan: unknown flags");
  if (q->reserved) return set_err(c, RL_E_INVALID, "gpu: rl_scan: reserved field not zero");
  if (q->unit_mask & ~rlhot::UNIT_BITS) return set_err(c, RL_E_INVALID, "gpu: rl_scan: unit_mask bit outside 1..4");
  const uint32_t n = q->n_prefixes;
  if (n > RL_FORGET_PREFIX_MAX) return set_err(c, RL_E_CAPACITY, "gpu: rl_scan: more than RL_FORGET_PREFIX_MAX prefixes");
  if (n && (!q->prefix_bytes || !q->prefix_off)) return set_err(c, RL_E_INVALID, "gpu: rl_scan: null prefix array");
  // (no empty prefix: n_prefixes == 0 is "every key")
  if (const int rc = stems_check<false, rlstem::ANY_LEN>(c, n, q->prefix_off, RL_FORGET_PREFIX_BYTES, "rl_scan prefix",
                                 "rl_scan prefix", "empty, or offsets decrease",
                                 "gpu: rl_scan: more than RL_FORGET_PREFIX_BYTES bytes of prefixes"))
    return rc;
  if ((q->flags & RL_SCAN_LIVE) && (q->now < 0 || q->now > (int64_t)NOW_MAX))
    return set_err(c, RL_E_TIME, "gpu: now out of range");
  if (out && !records_check(out)) return set_err(c, RL_E_INVALID, "gpu: null rl_records array");
  return RL_OK;
}

int eng_scan(Engine* c, const rl_scan_query* q, uint64_t* slot, rl_records* out, rl_scan_prefix_sum* by_prefix,
             rl_scan_info* info) {
  if (!c || !slot) return set_err(c, RL_E_INVALID, "gpu: null argument");
  if (const int rc = eng_scan_check(c, q, out)) return rc;
  if (*slot % RL_SCAN_TILE || *slot > c->nslots)
    return set_err(c, RL_E_INVALID, "gpu: rl_scan: cursor slot is no multiple of RL_SCAN_TILE, or beyond the shard");
  hipStream_t st;
  int64_t floor = 0;
  if (const int rc = call_begin(c, &st, &floor)) return rc;  // (the staging below is this synchronous call's own)
  if ((q->flags & RL_SCAN_LIVE) && q->now < floor) return set_err(c, RL_E_TIME, "gpu: now below the sweep floor");
  Engine::ScanStage& S = c->scan;
  const bool fresh = !S.pfx;
  if (fresh) {
    HIPCHK(c, dalloc(&S.pfx, (size_t)RL_FORGET_PREFIX_BYTES));
    HIPCHK(c, dalloc(&S.poff, (size_t)RL_FORGET_PREFIX_MAX + 1));
    HIPCHK(c, dalloc(&S.byp, (size_t)RL_FORGET_PREFIX_MAX * 3 + 1));
    HIPCHK(c, hipMemsetAsync(S.poff, 0, (RL_FORGET_PREFIX_MAX + 1) * 4, st));
  }
  const uint32_t np = q->n_prefixes, nbins = std::max(np, 1u);
  HIPCHK(c, prefix_upload(S.pfx, S.poff, q->prefix_bytes, q->prefix_off, np, fresh, st));
  HIPCHK(c, hipMemsetAsync(S.byp, 0, ((size_t)RL_FORGET_PREFIX_MAX * 3 + 1) * 8, st));
  uint32_t* d_err = reinterpret_cast<uint32_t*>(S.byp + RL_FORGET_PREFIX_MAX * 3);
  const ScanQueryDev dq{S.pfx, S.poff, np, q->flags, (q->flags & RL_SCAN_LIVE) ? (uint32_t)q->now : 0u, q->unit_mask};
  const TableDev t = table_view(c);
  const uint64_t total = rlscan::tiles_of(c->nslots), first = *slot / RL_SCAN_TILE;
  rl_scan_info sum{};
  sum.time_floor = floor;
  std::vector<rlscan::TileSum> h_sums;
  std::vector<uint64_t> h_base;
  auto slots_of = [&](uint64_t t0, uint64_t t1) {  // slots of the tiles [t0, t1)
    return std::min(t1 * RL_SCAN_TILE, c->nslots) - std::min(t0 * RL_SCAN_TILE, c->nslots);
  };
  uint64_t tile = first;
  if (!out) {
    // count only: one pass over the rest of the shard, which it covers whole
    for (; tile < total;) {
      const uint32_t nt = (uint32_t)std::min<uint64_t>(total - tile, 1u << 20);
      HIPCHK(c, scan_grow(&S.sums, &S.tile_cap, nt));
      launch_scan_count(t, c->nslots, tile, nt, dq, nullptr, S.sums, S.byp, st);
      HIPCHK(c, hipGetLastError());
      h_sums.resize(nt);
      HIPCHK(c, hipMemcpyAsync(h_sums.data(), S.sums, (size_t)nt * sizeof(rlscan::TileSum), hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
      for (const rlscan::TileSum& x : h_sums) {  // (no cut: a count has no 32-bit offsets to respect)
        sum.records += x.records;
        sum.stem_bytes += x.bytes;
        sum.keys += x.keys;
        sum.chains_lost += x.lost;
      }
      tile += nt;
    }
  } else {
    const uint64_t rec_cap = out->n, byte_cap = std::min<uint64_t>(out->stem_cap, rlscan::BYTES_MAX);
    // The spans start small and double: a small page then counts a few tiles,
    // not 2^22 slots, and a large one (the first span: as many tiles as the
    // page has records per RL_SCAN_TILE) is soon at full width.
    const uint32_t span0 = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(16, rec_cap / RL_SCAN_TILE), c->scan_span);
    for (uint32_t span = span0; tile < total; span = std::min(2 * span, c->scan_span)) {
      const uint32_t nt = (uint32_t)std::min<uint64_t>(total - tile, span);
      HIPCHK(c, scan_grow(&S.sums, &S.tile_cap, nt));
      HIPCHK(c, scan_grow(&S.cnt, &S.cnt_cap, (size_t)nt * RL_SCAN_TILE));
      launch_scan_count(t, c->nslots, tile, nt, dq, S.cnt, S.sums, nullptr, st);
      HIPCHK(c, hipGetLastError());
      h_sums.resize(nt);
      h_base.resize(nt);
      HIPCHK(c, hipMemcpyAsync(h_sums.data(), S.sums, (size_t)nt * sizeof(rlscan::TileSum), hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
      const rlscan::Cut cut =
          rlscan::plan(h_sums.data(), nt, rec_cap - sum.records, byte_cap - sum.stem_bytes, h_base.data());
      if (!cut.tiles && tile == first) {
        if (info) {
          *info = rl_scan_info{};
          info->need_records = h_sums[0].records;
          info->need_stem_bytes = h_sums[0].bytes;
          info->time_floor = floor;
        }
        return set_err(c, RL_E_CAPACITY,
                       "gpu: rl_scan: the first tile holds " + std::to_string(h_sums[0].records) + " records / " +
                           std::to_string(h_sums[0].bytes) + " stem bytes: larger than rl_records");
      }
      if (cut.records) {
        const uint64_t nrec = cut.records, nb = cut.bytes;
        HIPCHK(c, scan_grow(&S.base, &S.base_cap, cut.tiles));
        if (nrec > S.rec_cap) {  // (the seven record arrays grow together, each from the same capacity to the same)
          size_t grown = S.rec_cap;
          HIPCHK(c, records_arrays(S.o, nrec, [&](auto** p, size_t k) {
            size_t cap = S.rec_cap;
            const hipError_t e = scan_grow(p, &cap, k);
            grown = cap;
            return e;
          }));
          S.rec_cap = grown;
        }
        HIPCHK(c, scan_grow(&S.o.stem, &S.byte_cap, nb));
        HIPCHK(c, hipMemcpyAsync(S.base, h_base.data(), (size_t)cut.tiles * 8, hipMemcpyHostToDevice, st));
        launch_scan_write(t, c->nslots, tile, cut.tiles, dq, S.cnt, S.base, (uint32_t)sum.stem_bytes, S.o, (uint32_t)nrec,
                          (uint32_t)nb, S.byp, d_err, st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, records_to_host(S.o, nrec, nb, out, sum.records, sum.stem_bytes, st));
        HIPCHK(c, hipStreamSynchronize(st));  // (h_base and the staging are free again)
      }
      sum.records += cut.records;
      sum.stem_bytes += cut.bytes;
      sum.keys += cut.keys;
      sum.chains_lost += cut.lost;
      tile += cut.tiles;
      if (cut.tiles < nt) break;  // the next tile does not fit: the page is full
    }
  }
  unsigned long long h_byp[RL_FORGET_PREFIX_MAX * 3 + 1] = {};
  HIPCHK(c, hipMemcpyAsync(h_byp, S.byp, sizeof h_byp, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  uint64_t byp_records = 0;
  for (uint32_t p = 0; p < nbins; p++) byp_records += h_byp[p * 3 + 1];
  if ((uint32_t)h_byp[RL_FORGET_PREFIX_MAX * 3] || byp_records != sum.records)
    return set_err(c, RL_E_INTERNAL, "gpu: rl_scan wrote other than it counted");
  sum.slots_scanned = slots_of(first, tile);
  if (out) {
    out->n = (uint32_t)sum.records;
    out->stem_off[0] = 0;
    out->stem_off[sum.records] = (uint32_t)sum.stem_bytes;
  }
  if (by_prefix)
    for (uint32_t p = 0; p < nbins; p++) by_prefix[p] = rl_scan_prefix_sum{h_byp[p * 3], h_byp[p * 3 + 1], h_byp[p * 3 + 2]};
  if (info) *info = sum;
  *slot = std::min(tile * RL_SCAN_TILE, c->nslots);
  return RL_OK;
}

int eng_import_check(Engine* c, const rl_records* in) {
  if (!c || !in) return set_err(c, RL_E_INVALID, "gpu: null argument");
  const uint32_t n = in->n;
  if (n > c->cfg.max_batch) return set_err(c, RL_E_CAPACITY, "gpu: import exceeds configured max_batch");
  if (!n) return RL_OK;
  if (!in->stem_bytes || !in->stem_off || !in->unit || !in->ws || !in->count || !in->expire || !in->lc)
    return set_err(c, RL_E_INVALID, "gpu: null rl_records array");
  // (its own loop, as it was: a record's unit and ws are checked between its offsets and the next record's)
  if (in->stem_off[0] != 0) return set_err(c, RL_E_INVALID, "gpu: import stem offsets must start at 0");
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t a = in->stem_off[i], b = in->stem_off[i + 1];
    if (b <= a || b - a > 65535u)
      return set_err(c, RL_E_INVALID, "gpu: import record " + std::to_string(i) + ": stem offsets (1..65535 bytes)");
    const uint32_t u = in->unit[i];
    if (u < 1 || u > 4) return set_err(c, RL_E_INVALID, "gpu: import record " + std::to_string(i) + ": unit outside 1..4");
    if (in->ws[i] > NOW_MAX || in->ws[i] % div_of(u))
      return set_err(c, RL_E_INVALID,
                     "gpu: import record " + std::to_string(i) + ": ws is no window start of its unit (or > 2^32-172801)");
  }
  if (in->stem_off[n] > c->cfg.max_stem_bytes)
    return set_err(c, RL_E_CAPACITY, "gpu: import exceeds configured max_stem_bytes");
  return RL_OK;
}

int eng_import(Engine* c, const rl_records* in) {
  if (const int rc = eng_import_check(c, in)) return rc;
  RQ_SETTLE(c);
  const uint32_t n = in->n;
  if (!n) return RL_OK;
  // group the records by stem (a stem's records stay in arrival order): one
  // lane of k_import takes a stem with all its units
  std::vector<uint64_t> hash(n);
  for (uint32_t i = 0; i < n; i++) {
    uint64_t h = hash_stem_host(c->hk, in->stem_bytes + in->stem_off[i], in->stem_off[i + 1] - in->stem_off[i]);
    if ((uint32_t)(h >> 32) == KEY_DUP) h = ((uint64_t)(KEY_DUP - 1u) << 32) | (uint32_t)h;  // (as k_prepare homes it)
    hash[i] = h;
  }
  auto stem_cmp = [&](uint32_t x, uint32_t y) {
    const uint32_t lx = in->stem_off[x + 1] - in->stem_off[x], ly = in->stem_off[y + 1] - in->stem_off[y];
    if (lx != ly) return lx < ly ? -1 : 1;
    return memcmp(in->stem_bytes + in->stem_off[x], in->stem_bytes + in->stem_off[y], lx);
  };
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    if (hash[x] != hash[y]) return hash[x] < hash[y];
    const int k = stem_cmp(x, y);
    return k ? k < 0 : x < y;
  });
  std::vector<ImportRec> rec(n);
  std::vector<uint32_t> gstart;
  std::vector<unsigned long long> ghash;
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t i = order[j];
    if (!j || hash[i] != hash[order[j - 1]] || stem_cmp(i, order[j - 1])) {
      gstart.push_back(j);
      ghash.push_back(hash[i]);
    }
    ImportRec& r = rec[j];
    r.off = in->stem_off[i];
    r.lu = (in->stem_off[i + 1] - in->stem_off[i]) | ((uint32_t)in->unit[i] << 16) |
           ((uint32_t)((in->flags ? in->flags[i] : 0) & RL_REC_CHAIN_LOST) << 24);
    r.ws = in->ws[i];
    r.count = in->count[i];
    r.expire = in->expire[i];
    r.lc = in->lc[i];
    r.pad[0] = r.pad[1] = 0;
  }
  gstart.push_back(n);
  const uint32_t ng = (uint32_t)ghash.size(), nb = in->stem_off[n];
  hipStream_t st;
  if (const int rc = call_begin(c, &st)) return rc;
  DevBufs mem;
  uint8_t* d_stem = nullptr;
  ImportRec* d_rec = nullptr;
  uint32_t *d_gs = nullptr, *d_err = nullptr;
  unsigned long long *d_gh = nullptr, *d_epoch = nullptr;
  HIPCHK(c, mem.get(&d_stem, (size_t)nb + 64));
  HIPCHK(c, mem.get(&d_rec, n));
  HIPCHK(c, mem.get(&d_gs, (size_t)ng + 1));
  HIPCHK(c, mem.get(&d_gh, ng));
  HIPCHK(c, mem.get(&d_epoch, LOG_PARTS));
  HIPCHK(c, mem.get(&d_err, 1));
  HIPCHK(c, hipMemcpyAsync(d_stem, in->stem_bytes, nb, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_rec, rec.data(), (size_t)n * sizeof(ImportRec), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_gs, gstart.data(), ((size_t)ng + 1) * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_gh, ghash.data(), (size_t)ng * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(d_err, 0, 4, st));
  launch_import(table_view(c), c->hk, d_stem, nb, d_rec, d_gs, d_gh, ng, d_epoch, d_err, st);
  HIPCHK(c, hipGetLastError());
  uint32_t e = 0;
  HIPCHK(c, hipMemcpyAsync(&e, d_err, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return map_err(c, e);
}

int eng_lookup_check(Engine* c, const rl_keys* in, const rl_key_state* out) {
  if (!c || !in || !out) return set_err(c, RL_E_INVALID, "gpu: null argument");
  const uint32_t n = in->n;
  if (n > c->cfg.max_batch) return set_err(c, RL_E_CAPACITY, "gpu: lookup exceeds configured max_batch");
  if (!n) return RL_OK;
  if (!in->stem_bytes || !in->stem_off || !in->unit || !in->now)
    return set_err(c, RL_E_INVALID, "gpu: null rl_keys array");
  if (!out->status || !out->found || !out->count || !out->expire || !out->lc)
    return set_err(c, RL_E_INVALID, "gpu: null rl_key_state array");
  // (an empty or over-long stem is that key's own status)
  return stems_check<true, rlstem::ANY_LEN>(c, n, in->stem_off, c->cfg.max_stem_bytes, "lookup stem", "lookup key",
                                            "stem offsets decrease", "gpu: lookup exceeds configured max_stem_bytes");
}

int eng_lookup(Engine* c, const rl_keys* in, rl_key_state* out) {
  if (const int rc = eng_lookup_check(c, in, out)) return rc;
  RQ_SETTLE(c);
  const uint32_t n = in->n;
  if (!n) return RL_OK;
  const uint32_t nb = in->stem_off[n];
  std::vector<uint32_t> now32(n);  // the clocks as the table keeps them
  for (uint32_t i = 0; i < n; i++)
    now32[i] = in->now[i] < 0 || in->now[i] > (int64_t)NOW_MAX ? LOOKUP_NOW_BAD : (uint32_t)in->now[i];
  hipStream_t st;  // (the staging below is the synchronous entry points': free once the batches are done)
  if (const int rc = call_begin(c, &st)) return rc;
  if (nb) HIPCHK(c, hipMemcpyAsync(c->d_stem, in->stem_bytes, nb, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->d_off, in->stem_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->d_unit, in->unit, n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->d_req, now32.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  const LookupDev q{n, c->d_off, c->d_unit, c->d_req, c->d_status, c->d_code, c->d_rem, c->d_reset, c->d_limit};
  launch_lookup(table_view(c), c->hk, params(c), c->s[0].time_floor, c->d_stem, nb, q, st);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out->status, q.status, n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out->found, q.found, n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out->count, q.count, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out->expire, q.expire, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out->lc, q.lc, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));  // (now32 lives until here)
  return RL_OK;
}

int eng_forget_check(Engine* c, const rl_stems* in) {
  if (!c || !in) return set_err(c, RL_E_INVALID, "gpu: null argument");
  if (in->flags & ~(RL_FORGET_PREFIX | RL_FORGET_DRY_RUN)) return set_err(c, RL_E_INVALID, "gpu: rl_forget: unknown flags");
  const bool prefix = in->flags & RL_FORGET_PREFIX;
  const uint32_t n = in->n;
  if (prefix ? n > RL_FORGET_PREFIX_MAX : n > c->cfg.max_batch)
    return set_err(c, RL_E_CAPACITY, prefix ? "gpu: rl_forget: more than RL_FORGET_PREFIX_MAX prefixes"
                                            : "gpu: rl_forget exceeds configured max_batch");
  if (!n) return RL_OK;
  if (!in->stem_bytes || !in->stem_off) return set_err(c, RL_E_INVALID, "gpu: null rl_stems array");
  // (no empty prefix either: there is no "flush everything")
  return stems_check<false, 65535u>(c, n, in->stem_off, prefix ? RL_FORGET_PREFIX_BYTES : c->cfg.max_stem_bytes,
                                    "rl_forget stem", "rl_forget entry", "stem offsets (1..65535 bytes)",
                                    prefix ? "gpu: rl_forget: more than RL_FORGET_PREFIX_BYTES bytes of prefixes"
                                           : "gpu: rl_forget exceeds configured max_stem_bytes");
}

int eng_forget(Engine* c, const rl_stems* in, uint32_t* removed, rl_forget_info* info) {
  if (const int rc = eng_forget_check(c, in)) return rc;
  RQ_SETTLE(c);
  if (info) *info = rl_forget_info{};
  const uint32_t n = in->n;
  if (!n) return RL_OK;
  const uint32_t nb = in->stem_off[n];
  const bool prefix = in->flags & RL_FORGET_PREFIX;
  const uint32_t dry = in->flags & RL_FORGET_DRY_RUN ? 1u : 0u;
  hipStream_t st;  // (the staging below is the synchronous entry points': free once the batches are done)
  if (const int rc = call_begin(c, &st)) return rc;
  unsigned long long* ctr = c->s[0].counters;  // (words 0..2: scratch of the synchronous calls, as rl_sweep's)
  HIPCHK(c, hipMemsetAsync(ctr, 0, 24, st));
  DevBufs mem;
  uint32_t* d_removed = c->d_rem;
  if (prefix) {
    uint8_t* d_pfx = nullptr;
    uint32_t* d_poff = nullptr;
    HIPCHK(c, mem.get(&d_pfx, (size_t)RL_FORGET_PREFIX_BYTES));
    HIPCHK(c, mem.get(&d_poff, (size_t)RL_FORGET_PREFIX_MAX + 1));
    HIPCHK(c, mem.get(&d_removed, (size_t)RL_FORGET_PREFIX_MAX));
    HIPCHK(c, prefix_upload(d_pfx, d_poff, in->stem_bytes, in->stem_off, n, true, st));
    HIPCHK(c, hipMemsetAsync(d_removed, 0, RL_FORGET_PREFIX_MAX * 4, st));
    launch_forget_scan(table_view(c), c->nslots, d_pfx, d_poff, n, dry, ctr, d_removed, st);
  } else {
    uint32_t* claim = nullptr;
    if (dry) {  // one bit per slot, for this call only: a dry run claims there what the real call claims in the tags
      const size_t words = (size_t)((c->nslots + 31) / 32);
      HIPCHK(c, mem.get(&claim, words));
      HIPCHK(c, hipMemsetAsync(claim, 0, words * 4, st));
    }
    HIPCHK(c, hipMemcpyAsync(c->d_stem, in->stem_bytes, nb, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->d_off, in->stem_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st));
    const ForgetDev q{n, c->d_off, d_removed, ctr, claim, dry};
    launch_forget_keys(table_view(c), c->hk, c->d_stem, nb, q, st);
  }
  HIPCHK(c, hipGetLastError());
  unsigned long long h[3] = {};
  HIPCHK(c, hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
  if (removed) HIPCHK(c, hipMemcpyAsync(removed, d_removed, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (!dry && h[2]) c->arena_forgotten = true;
  if (info) {
    info->slots_scanned = prefix ? c->nslots : 0;
    info->keys = h[0];
    info->keys_with_history = h[1];
    info->arena_bytes = h[2] * 16;
  }
  return RL_OK;
}

// ---------------------------------------------------------------------------
// The three resizes on one engine, in the two steps rl_engine.h describes.
// rl_resize: the placement scan puts every live key into the new table; the
// commit re-points the history log and swaps slots / nslots.
// ---------------------------------------------------------------------------
int eng_resize_check(Engine* c, uint64_t table_slots) {
  if (!c) return set_err(c, RL_E_INVALID, "gpu: null ctx");
  if (table_slots < 2 || (table_slots & (table_slots - 1)) || table_slots > (1ull << 32))
    return set_err(c, RL_E_INVALID, "gpu: rl_resize: table_slots must be a power of two in [2, 2^32]");
  return RL_OK;
}

int eng_resize_place(Engine* c, uint64_t table_slots, ResizePlan* p) {
  if (!p) return set_err(c, RL_E_INVALID, "gpu: null argument");
  *p = ResizePlan{};
  if (const int rc = eng_resize_check(c, table_slots)) return rc;
  hipStream_t st;
  if (const int rc = call_begin(c, &st)) return rc;
  hipError_t e = p->mem.get(&p->slots, table_slots);
  if (e == hipSuccess) e = p->mem.get(&p->map, c->nslots);
  if (e == hipSuccess) e = p->mem.get(&p->ctr, RESIZE_CTR_WORDS);
  if (e == hipSuccess) e = hipMemsetAsync(p->slots, 0, table_slots * sizeof(Slot), st);
  if (e == hipSuccess) e = hipMemsetAsync(p->ctr, 0, RESIZE_CTR_WORDS * 8, st);
  unsigned long long h[RESIZE_CTR_WORDS] = {};
  if (e == hipSuccess) {
    launch_resize_place(table_view(c), c->hk, c->nslots, p->slots, table_slots, p->map, p->ctr, st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, p->ctr, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // (an allocation that failed is this call's error, not the next one's)
    return plan_fail(c, p, RL_E_HIP, std::string("gpu: rl_resize: ") + hipGetErrorString(e) +
                                         " (the old and the new table coexist during the call)");
  }
  if (h[2])
    return plan_fail(c, p, RL_E_INTERNAL, "gpu: rl_resize: " + std::to_string(h[2]) +
                                                " live slots whose stem does not hash to their tag and place");
  if (h[3])
    return plan_fail(c, p, RL_E_TABLE_FULL,
                       "gpu: rl_resize: " + std::to_string(h[3]) + " of " + std::to_string(h[0] + h[3]) +
                           " keys find no free slot within their probe window of a table of " +
                           std::to_string(table_slots) + " slots");
  p->nslots = table_slots;
  p->info.slots_before = c->nslots;
  p->info.slots_after = table_slots;
  p->info.keys = h[0];
  p->info.tombstones_dropped = h[1];
  p->info.longest_probe = (uint32_t)h[4];
  return RL_OK;
}

int eng_resize_commit(Engine* c, ResizePlan* p) {
  if (!c || !p || !p->slots) return set_err(c, RL_E_INVALID, "gpu: rl_resize: nothing placed");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream;
  unsigned long long relinked = 0;
  launch_resize_relink(table_view(c), c->nslots, p->map, p->ctr, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&relinked, p->ctr + 5, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess)  // (a failed kernel: the device's state is lost either way)
    return plan_fail(c, p, RL_E_HIP, std::string("gpu: rl_resize: re-link: ") + hipGetErrorString(e));
  p->info.log_entries_relinked = relinked;
  p->mem.swap(&c->slots, &p->slots);
  c->nslots = p->nslots;
  c->cfg.table_slots = p->nslots;
  plan_finish(c, p);
  return RL_OK;
}

// ---------------------------------------------------------------------------
// rl_resize_history: the placement copies the entries on live chains into the
// new log and fills the head map; the commit stores the new chain heads into
// the slots, restarts the append counters at the entries placed (the log_ctr
// allocation stays: k_b_begin reads it; its line of lost / refused counts is
// left alone) and swaps log / log_cap.
// ---------------------------------------------------------------------------
int eng_relog_check(Engine* c, uint64_t history_entries) {
  if (!c) return set_err(c, RL_E_INVALID, "gpu: null ctx");
  if (!history_entries || !log_entries_fit(history_entries, LOG_PARTS, LOG_PART_MAX))
    return set_err(c, RL_E_INVALID, "gpu: rl_resize_history: history_entries must be in [1, 2^31]");
  return RL_OK;
}

int eng_relog_place(Engine* c, uint64_t history_entries, RelogPlan* p) {
  if (!p) return set_err(c, RL_E_INVALID, "gpu: null argument");
  *p = RelogPlan{};
  if (const int rc = eng_relog_check(c, history_entries)) return rc;
  hipStream_t st;
  if (const int rc = call_begin(c, &st)) return rc;
  const uint32_t cap = (uint32_t)log_part_cap(history_entries, c->cfg.max_batch, LOG_PARTS, LOG_PART_MAX);
  std::vector<unsigned long long> old;
  HIPCHK(c, log_ctr_get(c, old, nullptr));
  hipError_t e = p->mem.get(&p->log, (size_t)LOG_PARTS * cap);
  if (e == hipSuccess) e = p->mem.get(&p->map, c->nslots);
  if (e == hipSuccess) e = p->mem.get(&p->ctr, RELOG_CTR_WORDS);
  // (the new log is not cleared: entries are written before any chain points at them, as at rl_create)
  if (e == hipSuccess) e = hipMemsetAsync(p->ctr, 0, RELOG_CTR_WORDS * 8, st);
  std::vector<unsigned long long> h(RELOG_CTR_WORDS);
  if (e == hipSuccess) {
    launch_relog_place(table_view(c), c->nslots, p->log, cap, p->map, p->ctr, st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), p->ctr, h.size() * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // (an allocation that failed is this call's error, not the next one's)
    return plan_fail(c, p, RL_E_HIP, std::string("gpu: rl_resize_history: ") + hipGetErrorString(e) +
                                         " (the old log, the new log and 4 bytes per slot coexist during the call)");
  }
  const unsigned long long* stats = h.data() + RELOG_CTR_STATS;
  uint64_t fill_max = 0;
  p->fill.resize(LOG_PARTS);
  for (uint32_t k = 0; k < LOG_PARTS; k++) {
    p->fill[k] = h[(size_t)k * LOG_CTR_STRIDE];
    fill_max = std::max<uint64_t>(fill_max, p->fill[k]);
  }
  if (stats[4] || fill_max > cap)
    return plan_fail(c, p, RL_E_CAPACITY,
                       "gpu: rl_resize_history: a partition of the new log was asked for " + std::to_string(fill_max) +
                           " entries and holds " + std::to_string(cap) + " (history_entries of at least " +
                           std::to_string(fill_max * LOG_PARTS) + " would fit)");
  p->log_cap = cap;
  p->info.entries_before = (uint64_t)LOG_PARTS * c->log_cap;
  p->info.entries_after = (uint64_t)LOG_PARTS * cap;
  for (unsigned long long k : old) {
    p->appended += k;
    p->info.written_before += std::min<uint64_t>(k, c->log_cap);
  }
  p->info.entries_kept = stats[1];
  p->info.entries_dropped = p->info.written_before - stats[1];
  p->info.chains = stats[0];
  p->info.chains_lost = stats[2];
  p->info.longest_chain = (uint32_t)stats[3];
  p->info.fill_max = fill_max;
  return RL_OK;
}

int eng_relog_commit(Engine* c, RelogPlan* p) {
  if (!c || !p || !p->log) return set_err(c, RL_E_INVALID, "gpu: rl_resize_history: nothing placed");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream;
  std::vector<unsigned long long> hc((size_t)LOG_PARTS * LOG_CTR_STRIDE, 0ull);
  uint64_t placed = 0;
  for (uint32_t k = 0; k < LOG_PARTS; k++) {
    hc[(size_t)k * LOG_CTR_STRIDE] = p->fill[k];
    placed += p->fill[k];
  }
  launch_relog_commit(c->slots, c->nslots, p->map, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(c->log_ctr, hc.data(), hc.size() * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess)  // (a failed kernel: the device's state is lost either way)
    return plan_fail(c, p, RL_E_HIP, std::string("gpu: rl_resize_history: commit: ") + hipGetErrorString(e));
  c->hist_base += p->appended - placed;  // (history_appended stays where it was)
  p->mem.swap(&c->log, &p->log);
  c->log_cap = p->log_cap;
  c->cfg.history_entries = (uint64_t)LOG_PARTS * p->log_cap;
  plan_finish(c, p);
  return RL_OK;
}

// ---------------------------------------------------------------------------
// rl_resize_arena: a new pair of arenas (the live one and the sweep's
// compaction target), the used bytes copied device to device. Offsets are
// kept, so no slot changes; the cursor (counters[4]) stays.
// ---------------------------------------------------------------------------
int eng_arena_check(Engine* c, uint64_t arena_bytes) {
  if (!c) return set_err(c, RL_E_INVALID, "gpu: null ctx");
  if (!arena_bytes || (arena_bytes & 15u) || arena_bytes / 16 > (1ull << 32))
    return set_err(c, RL_E_INVALID, "gpu: rl_resize_arena: arena_bytes must be a multiple of 16 in [16, 2^36]");
  return RL_OK;
}

int eng_arena_place(Engine* c, uint64_t arena_bytes, ArenaPlan* p) {
  if (!p) return set_err(c, RL_E_INVALID, "gpu: null argument");
  *p = ArenaPlan{};
  if (const int rc = eng_arena_check(c, arena_bytes)) return rc;
  hipStream_t st;
  if (const int rc = call_begin(c, &st)) return rc;
  unsigned long long used16 = 0;
  HIPCHK(c, hipMemcpyAsync(&used16, c->s[0].counters + 4, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (used16 > arena_bytes / 16)
    return set_err(c, RL_E_ARENA_FULL, "gpu: rl_resize_arena: " + std::to_string(used16 * 16) +
                                           " bytes are in use (rl_sweep compacts the arena)");
  hipError_t e = p->mem.get(&p->arena, arena_bytes);
  if (e == hipSuccess) e = p->mem.get(&p->arena2, arena_bytes);
  if (e == hipSuccess && used16) e = hipMemcpyAsync(p->arena, c->arena, used16 * 16, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return plan_fail(c, p, RL_E_HIP, std::string("gpu: rl_resize_arena: ") + hipGetErrorString(e) +
                                         " (the old and the new pair of arenas coexist during the call)");
  }
  p->cap16 = arena_bytes / 16;
  return RL_OK;
}

void eng_arena_commit(Engine* c, ArenaPlan* p) {
  p->mem.swap(&c->arena, &p->arena);
  p->mem.swap(&c->arena2, &p->arena2);
  c->arena_cap16 = p->cap16;
  c->cfg.arena_bytes = p->cap16 * 16;
  eng_plan_abort(c, p);
}

}  // namespace rl
