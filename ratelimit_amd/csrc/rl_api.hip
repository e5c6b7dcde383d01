// rl_api.hip — the extern "C" boundary of libratelimit_hip.so
// (include/ratelimit_hip.h).
//
// A ctx holds one engine per table shard (rl_engine.h: HBM table, pipeline
// buffers, streams). With one shard every entry point is the engine's own.
// With rl_config.n_shards > 1 the table is hash-sharded over the shards'
// devices inside this one process (the reference's single service process
// scaled out over a Redis cluster, src/redis/driver_impl.go:108-126; here the
// cgo adapter still drives one ctx). Each shard then also has a router
// (rl_comm.hip) and a worker thread; the routers form an in-process loopback
// world, so a multi-shard ctx runs exactly the protocol of one process per
// GPU (partition by owner, counts, records and stems, owner pipelines,
// results and stats, scatter), each shard on its own thread:
//
//   host batches (rl_do_limit, rl_do_limit_host_async): the batch is cut into
//     one request-aligned slice per shard; each shard's router copies its
//     slice over ITS device's PCIe link, partitions it and exchanges with the
//     others over xGMI (peer copies); the answers cross back per slice, and
//     the per-shard stats deltas are summed on the host;
//   device batches (rl_do_limit_async, memory of shard 0's GPU): shard 0's
//     router takes the whole batch and the others submit empty slices.
//
// The caller's thread only hands each batch to the workers and waits until
// they have ENQUEUED it (never for the GPU); rl_synchronize completes the
// in-flight batches (a collective step of the routers).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ratelimit_hip.h"
#include "rl_comm.h"
#include "rl_device.h"
#include "rl_engine.h"
#include "rl_kernels.h"
#include "rl_shard_split.h"

using namespace rl;

namespace {

constexpr uint32_t MAX_LOCAL_SHARDS = 16;

// One shard's worker: runs its router's collective steps on its own thread.
// (A ctx of one shard has no thread; rl_resize and rl_resize_history still keep
// its plan in w[0], placed on the caller's thread.)
struct ShardWorker {
  enum Job { IDLE, BATCH, SYNC, RESIZE, FORGET, RELOG, EXIT };
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  Job job = IDLE;
  rl_batch in{};
  rl_result out{};
  CommIO io{};
  hipStream_t caller = nullptr;
  uint64_t rs_slots = 0;  // RESIZE: the new slot count, and what the shard placed
  ResizePlan rs_plan;
  uint64_t rl_entries = 0;  // RELOG: the new history_entries, and what the shard placed
  RelogPlan rl_plan;
  const rl_stems* fg_in = nullptr;  // FORGET: the call's prefixes, and this shard's answer
  uint32_t fg_removed[RL_FORGET_PREFIX_MAX] = {};
  rl_forget_info fg_info{};
  int rc = RL_OK;
};

// Stats of a host batch in flight: each shard's deltas land in a pinned ring
// entry (slot = the routers' slot of the batch); they are summed into the
// caller's out->stats once the batch is complete.
struct PendingStats {
  bool used = false;
  uint64_t* out = nullptr;
  uint32_t m = 0;
};

}  // namespace

struct rl_ctx {
  rl_config cfg;
  uint32_t n = 1;
  Engine* e[MAX_LOCAL_SHARDS] = {};
  CommRouter* comm = nullptr;  // rl_comm_init: multi-process routing (single-shard ctx)
  std::string last_error;
  // shards of this ctx (n > 1; w[0] also holds a one-shard ctx's resize plans)
  CommRouter* r[MAX_LOCAL_SHARDS] = {};
  ShardWorker w[MAX_LOCAL_SHARDS];
  std::mutex done_mu;
  std::condition_variable done_cv;
  uint32_t busy = 0;
  uint32_t batch_no = 0;                      // batches submitted (router slot = batch_no % slots)
  std::vector<PendingStats> pend;             // [slots]
  unsigned long long* stats_ring = nullptr;   // pinned [slots][n][stats_cap]
  uint32_t stats_cap = 0;
};

namespace {

thread_local std::string g_api_err;

int fail(rl_ctx* c, int code, const std::string& msg) {
  if (c) c->last_error = msg;
  else g_api_err = msg;
  return code;
}

// An engine's failure, surfaced through the ctx.
int from_engine(rl_ctx* c, Engine* e, int rc) {
  if (rc && c->n > 1) c->last_error = eng_last_error(e);
  return rc;
}

#define API_HIP(c, expr)                                                                        \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return fail((c), RL_E_HIP, std::string("gpu: ") + #expr + ": " + hipGetErrorString(_e));  \
  } while (0)

uint32_t owner_of_host(uint64_t h, uint32_t n) { return (uint32_t)(((uint64_t)(uint32_t)h * n) >> 32); }

// The sink rule: a maintenance call's own refusal goes where rl_last_error
// reads it, a one-shard ctx's engine or the ctx. (rl_restore, rl_import,
// rl_lookup, rl_export_range and older calls use plain fail: DESIGN.md §11.)
int fail_call(rl_ctx* c, int code, const std::string& msg) {
  return c && c->n == 1 ? eng_fail(c->e[0], code, msg) : fail(c, code, msg);
}

// A call's stem list split by owning shard. False: an entry's offsets decrease.
bool split_by_owner(rl_ctx* c, uint32_t n, const uint8_t* stem_bytes, const uint32_t* stem_off,
                    std::vector<rlsplit::Sub>* out) {
  const HashKey& hk = c->e[0]->hk;
  const uint32_t N = c->n;
  auto owner = [&](const uint8_t* s, uint32_t len) { return owner_of_host(hash_stem_host(hk, s, len), N); };
  return rlsplit::split(n, stem_bytes, stem_off, N, owner, out);
}

// The three resizes share one shape: these refusals and the size's check on
// shard 0; the shards settle; every shard places its new memory beside the old
// (table and log on the shards' workers, or here for a one-shard ctx; the arena
// inline: small); all commit or all abort.
int resize_refused(rl_ctx* c, const char* name) {
  if (!c) return fail_call(c, RL_E_INVALID, "gpu: null ctx");
  if (c->comm) return fail_call(c, RL_E_INVALID, std::string("gpu: ") + name + " is not for a ctx that joined a communicator");
  return RL_OK;
}

// rc: the placements'. plan(j): shard j's plan; commit(engine, plan) -> rl_status (and takes the plan's info).
template <typename PlanOf, typename Commit>
int resize_commit_all(rl_ctx* c, int rc, PlanOf plan, Commit commit) {
  for (uint32_t j = 0; j < c->n && !rc; j++) rc = from_engine(c, c->e[j], commit(c->e[j], plan(j)));
  for (uint32_t j = 0; j < c->n; j++) eng_plan_abort(c->e[j], plan(j));  // (what was not committed)
  return rc;
}

void worker_main(rl_ctx* c, uint32_t j) {
  (void)hipSetDevice(c->cfg.shard_device[j]);
  ShardWorker& w = c->w[j];
  for (;;) {
    ShardWorker::Job job;
    {
      std::unique_lock<std::mutex> l(w.mu);
      w.cv.wait(l, [&] { return w.job != ShardWorker::IDLE; });
      job = w.job;
    }
    if (job == ShardWorker::EXIT) return;
    int rc = RL_OK;
    if (job == ShardWorker::BATCH) {
      rc = comm_do_limit(c->r[j], c->e[j], &w.in, &w.out, w.caller, &w.io);
    } else if (job == ShardWorker::RESIZE) {  // (the placement only: rl_resize commits once every shard has placed)
      rc = eng_resize_place(c->e[j], w.rs_slots, &w.rs_plan);
    } else if (job == ShardWorker::RELOG) {  // (likewise: rl_resize_history commits once every shard has placed)
      rc = eng_relog_place(c->e[j], w.rl_entries, &w.rl_plan);
    } else if (job == ShardWorker::FORGET) {  // (prefix mode: every shard scans its own table)
      rc = eng_forget(c->e[j], w.fg_in, w.fg_removed, &w.fg_info);
    } else {  // SYNC: the pending batch (collective), the router's streams, then the engine's error words
      rc = comm_synchronize(c->r[j], c->e[j]);
      const int re = eng_synchronize(c->e[j]);
      if (!rc) rc = re;
    }
    {
      std::lock_guard<std::mutex> l(w.mu);
      w.rc = rc;
      w.job = ShardWorker::IDLE;
    }
    {
      std::lock_guard<std::mutex> l(c->done_mu);
      c->busy--;
    }
    c->done_cv.notify_all();
  }
}

// Hand every shard its job (set up by the caller) and wait until all have
// returned from it; the first failing shard's status and message.
int run_shards(rl_ctx* c, ShardWorker::Job job) {
  {
    std::lock_guard<std::mutex> l(c->done_mu);
    c->busy = c->n;
  }
  for (uint32_t j = 0; j < c->n; j++) {
    {
      std::lock_guard<std::mutex> l(c->w[j].mu);
      c->w[j].job = job;
    }
    c->w[j].cv.notify_one();
  }
  {
    std::unique_lock<std::mutex> l(c->done_mu);
    c->done_cv.wait(l, [&] { return c->busy == 0; });
  }
  for (uint32_t j = 0; j < c->n; j++)
    if (c->w[j].rc) return fail(c, c->w[j].rc, eng_last_error(c->e[j]));
  return RL_OK;
}

void stop_shards(rl_ctx* c) {
  for (uint32_t j = 0; j < c->n; j++) {
    if (!c->w[j].th.joinable()) continue;
    {
      std::lock_guard<std::mutex> l(c->w[j].mu);
      c->w[j].job = ShardWorker::EXIT;
    }
    c->w[j].cv.notify_one();
    c->w[j].th.join();
  }
}

// The summed stats of the host batch that used ring entry s (its shards'
// slots are complete once their done events fired).
int finalize_stats(rl_ctx* c, uint32_t s, bool keep) {
  PendingStats& P = c->pend[s];
  if (!P.used) return RL_OK;
  P.used = false;
  for (uint32_t j = 0; j < c->n; j++) {
    const int rc = comm_wait_slot(c->r[j], c->e[j], s);
    if (rc) return from_engine(c, c->e[j], rc);
  }
  if (!keep || !P.out) return RL_OK;
  for (uint32_t i = 0; i < P.m; i++) {
    unsigned long long v = 0;
    for (uint32_t j = 0; j < c->n; j++) v += c->stats_ring[((size_t)s * c->n + j) * c->stats_cap + i];
    P.out[i] = v;
  }
  return RL_OK;
}

// keep_stats false (rl_destroy): the shards complete, but no caller memory is
// written (the caller may have freed a pending batch's outputs).
int synchronize_all(rl_ctx* c, bool keep_stats = true) {
  if (c->n > 1) {
    const int rc = run_shards(c, ShardWorker::SYNC);
    const std::string msg = c->last_error;
    for (uint32_t s = 0; s < c->pend.size(); s++) {
      const int fr = finalize_stats(c, s, keep_stats && rc == RL_OK);
      if (fr && !rc) return fr;
    }
    if (rc) c->last_error = msg;
    return rc;
  }
  int comm_rc = RL_OK;
  std::string comm_msg;
  if (c->comm) {  // (collective on a routed ctx: it completes the pending batch)
    comm_rc = comm_synchronize(c->comm, c->e[0]);
    if (comm_rc) comm_msg = eng_last_error(c->e[0]);
  }
  if (comm_rc) {
    // the engine's own words are collected (and cleared) too; the router's
    // failure is the one reported
    (void)eng_synchronize(c->e[0]);
    return eng_fail(c->e[0], comm_rc, comm_msg);
  }
  return eng_synchronize(c->e[0]);
}

// One batch through the shards: host (slices over every shard's link) or
// device (memory of shard 0's GPU: shard 0 takes it whole). cb: a compact host
// batch (in then carries only its sizes), cut at request boundaries.
int shards_submit(rl_ctx* c, const rl_batch* in, rl_result* out, bool host, hipStream_t caller,
                  const rl_batch_compact* cb = nullptr, const rl_batch_prefixed* pb = nullptr) {
  const uint32_t N = c->n, n = in->n, nq = in->n_requests;
  const uint32_t slots = (uint32_t)c->pend.size(), s = c->batch_no % slots;
  // the batch that used this slot of the routers is complete: its stats first
  int rc = finalize_stats(c, s, true);
  if (rc) return rc;
  const uint32_t m = in->n_rules * RL_NUM_STATS;
  if (host && m > c->stats_cap) {  // a larger stats ring: every pending batch completed and finalized first
    // (the last batch's second half runs only at the next call or a sync:
    // finalizing its ring entry before that read zeros)
    if ((rc = synchronize_all(c))) return rc;
    if (c->stats_ring) (void)hipHostFree(c->stats_ring);
    c->stats_ring = nullptr;
    c->stats_cap = 0;
    API_HIP(c, hipHostMalloc((void**)&c->stats_ring, (size_t)slots * N * m * 8));
    c->stats_cap = m;
  }
  if (host && c->stats_ring && c->stats_cap)  // (a slice that fails never writes its part: no stale deltas)
    memset(c->stats_ring + (size_t)s * N * c->stats_cap, 0, (size_t)N * c->stats_cap * 8);
  // request-aligned cuts of about n / N descriptors
  uint32_t d[MAX_LOCAL_SHARDS + 1], q[MAX_LOCAL_SHARDS + 1];
  d[0] = 0;
  q[0] = 0;
  d[N] = n;
  q[N] = nq;
  const uint32_t* first = cb ? reinterpret_cast<const uint32_t*>(cb->buf + cb->req_first) : nullptr;
  // a prefix-shared batch is cut at request tiles: the index holds each tile's first descriptor
  const uint32_t tiles = pb ? (nq + RL_PREFIXED_TILE - 1) / RL_PREFIXED_TILE : 0;
  const uint32_t* pix = pb ? reinterpret_cast<const uint32_t*>(pb->buf + pb->index) : nullptr;
  uint32_t t[MAX_LOCAL_SHARDS + 1];
  t[0] = 0;
  t[N] = tiles;
  for (uint32_t j = 1; j < N; j++) {
    if (pb) {  // (entries are checked against the sections on the device; clamp so slices stay ordered)
      t[j] = (uint32_t)((uint64_t)tiles * j / N);
      q[j] = std::min(t[j] * RL_PREFIXED_TILE, nq);
      d[j] = std::min(std::max(pix[4ull * t[j]], d[j - 1]), n);
      continue;
    }
    if (cb) {  // (about nq / N requests each; req_first was checked to lie in [0, n] by nobody yet: clamp)
      q[j] = std::max(q[j - 1], (uint32_t)((uint64_t)nq * j / N));
      d[j] = std::min(std::max(first[q[j]], d[j - 1]), n);
      continue;
    }
    uint32_t x = host ? (uint32_t)((uint64_t)n * j / N) : n;
    if (x < d[j - 1]) x = d[j - 1];
    while (x > 0 && x < n && in->req_idx[x] == in->req_idx[x - 1]) x++;
    d[j] = x;
    q[j] = x < n ? std::min(in->req_idx[x], nq) : nq;
    if (q[j] < q[j - 1]) q[j] = q[j - 1];
  }
  for (uint32_t j = 0; j < N; j++) {
    ShardWorker& w = c->w[j];
    w.caller = j == 0 ? caller : nullptr;
    w.io = CommIO{};
    w.in = *in;
    w.out = rl_result{};
    if (host && (cb || pb)) {
      const uint32_t a = d[j], b = d[j + 1];
      w.in = rl_batch{};
      w.in.n = b - a;
      w.in.n_requests = q[j + 1];  // (absolute: the slice's first request is q[j])
      w.in.n_rules = in->n_rules;
      w.out.code = out->code + a;
      w.out.limit_remaining = out->limit_remaining + a;
      w.out.reset_s = out->reset_s ? out->reset_s + a : nullptr;
      w.out.status = out->status ? out->status + a : nullptr;
      w.io.host = true;
      w.io.cb = cb;
      w.io.pb = pb;
      w.io.t0 = t[j];
      w.io.t1 = t[j + 1];
      w.io.da = a;
      w.io.qa = q[j];
      w.io.stats_host = m ? c->stats_ring + ((size_t)s * N + j) * c->stats_cap : nullptr;
    } else if (host) {
      const uint32_t a = d[j], b = d[j + 1];
      w.in.n = b - a;
      w.in.n_requests = q[j + 1];  // (absolute: the slice's first request is q[j])
      w.in.stem_off = in->stem_off + a;
      w.in.req_idx = in->req_idx + a;
      w.in.unit = in->unit + a;
      w.in.flags = in->flags + a;
      w.in.limit = in->limit + a;
      w.in.hits = in->hits + a;
      w.in.rule_id = in->rule_id + a;
      w.out.code = out->code ? out->code + a : nullptr;
      w.out.limit_remaining = out->limit_remaining ? out->limit_remaining + a : nullptr;
      w.out.reset_s = out->reset_s ? out->reset_s + a : nullptr;
      w.out.status = out->status ? out->status + a : nullptr;
      w.io.host = true;
      w.io.da = a;
      w.io.qa = q[j];
      w.io.stats_host = m ? c->stats_ring + ((size_t)s * N + j) * c->stats_cap : nullptr;
    } else if (j == 0) {
      w.out = *out;
    } else {  // an empty slice (the exchange is collective)
      w.in = rl_batch{};
      w.in.n_rules = in->n_rules;
    }
  }
  c->batch_no++;
  rc = run_shards(c, ShardWorker::BATCH);
  if (rc) return rc;
  if (host) {
    c->pend[s].used = true;
    c->pend[s].out = out->stats;
    c->pend[s].m = out->stats ? m : 0;
  }
  return RL_OK;
}

// Settle a multi-shard or routed ctx before a call that changes the table
// (on a routed ctx this makes the call collective, like rl_synchronize).
int settle(rl_ctx* c) { return (c->comm || c->n > 1) ? synchronize_all(c) : RL_OK; }
// Before a read-only getter: the shards of one ctx complete their batches
// (in-process, no peer to wait for); a routed ctx is not settled, since its
// pending batch's second half is a collective exchange and one rank polling
// its gauges would block on its peers. The engine getters order after every
// batch already enqueued on the engine, so a routed ctx's getters see all
// batches but the last one submitted.
int settle_local(rl_ctx* c) { return c->n > 1 ? synchronize_all(c) : RL_OK; }

constexpr uint64_t MSNAP_MAGIC = 0x31304853414e534cull;  // "LSNASH01": one image per shard

}  // namespace

extern "C" {

uint32_t rl_abi_version(void) { return RL_ABI_VERSION; }

const char* rl_last_error(const rl_ctx* c) {
  if (!c) return g_api_err.c_str();
  return c->n == 1 ? eng_last_error(c->e[0]) : c->last_error.c_str();
}

rl_ctx* rl_create(const rl_config* cfg_in, char* err, size_t errlen) {
  auto bad = [&](const std::string& m) -> rl_ctx* {
    if (err && errlen) snprintf(err, errlen, "%s", m.c_str());
    g_api_err = m;
    return nullptr;
  };
  if (!cfg_in) return bad("gpu: null config");
  rl_config cfg = *cfg_in;
  const uint32_t n = cfg.n_shards ? cfg.n_shards : 1;
  if (n > MAX_LOCAL_SHARDS) return bad("gpu: n_shards must be at most 16");
  rl_ctx* c = new rl_ctx();
  if (n == 1) {
    cfg.n_shards = 1;
    c->e[0] = eng_create(&cfg, err, errlen);
    if (!c->e[0]) {
      delete c;
      return nullptr;
    }
    c->cfg = c->e[0]->cfg;
    return c;
  }
  // one key for every shard: the owner of a stem is a function of its hash
  while (!cfg.hash_seed) {
    std::random_device rd;
    cfg.hash_seed = ((uint64_t)rd() << 32) ^ rd();
  }
  if (!cfg.max_batch) cfg.max_batch = 1u << 20;
  if (!cfg.max_requests) cfg.max_requests = cfg.max_batch;
  if (!cfg.max_rules) cfg.max_rules = 65536;
  if (!cfg.max_stem_bytes) cfg.max_stem_bytes = 128u * cfg.max_batch;
  c->n = n;
  c->cfg = cfg;
  for (uint32_t j = 0; j < n; j++) {
    rl_config ec = cfg;
    ec.n_shards = 1;
    ec.device = cfg.shard_device[j];
    // the shards' router keeps stats per source slice (rule' = source x n_rules + rule):
    // an owner needs n x max_rules rows for batches of max_rules rules
    ec.max_rules = cfg.max_rules * n;
    c->e[j] = eng_create(&ec, err, errlen);
    if (!c->e[j]) {
      const std::string m = g_api_err = (err && errlen) ? std::string(err) : std::string("gpu: shard creation failed");
      rl_destroy(c);
      return bad(m);
    }
  }
  c->cfg = c->e[0]->cfg;
  c->cfg.n_shards = n;
  c->cfg.max_rules = cfg.max_rules;  // (what a batch may carry; the shards hold n x as many rows)
  for (uint32_t j = 0; j < MAX_LOCAL_SHARDS; j++) c->cfg.shard_device[j] = cfg.shard_device[j];
  // every pair of distinct shard devices talks directly over xGMI
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t j = 0; j < n; j++) {
      const int di = cfg.shard_device[i], dj = cfg.shard_device[j];
      int can = 0;
      if (di == dj || hipDeviceCanAccessPeer(&can, di, dj) != hipSuccess || !can) continue;
      (void)hipSetDevice(di);
      const hipError_t e = hipDeviceEnablePeerAccess(dj, 0);
      (void)hipGetLastError();
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
        rl_destroy(c);
        return bad("gpu: peer access between shard devices failed");
      }
    }
  // the shards' routers: one in-process loopback world
  uint8_t id[RL_COMM_ID_BYTES];
  std::string cerr;
  if (comm_loopback_id(id, &cerr)) {
    rl_destroy(c);
    return bad(cerr);
  }
  for (uint32_t j = 0; j < n; j++) {
    c->r[j] = comm_create(c->e[j], n, j, id, &cerr);
    if (!c->r[j]) {
      rl_destroy(c);
      return bad(cerr);
    }
  }
  c->pend.assign(comm_slots(), PendingStats{});
  for (uint32_t j = 0; j < n; j++) c->w[j].th = std::thread(worker_main, c, j);
  return c;
}

void rl_destroy(rl_ctx* c) {
  if (!c) return;
  if (c->comm) comm_destroy(c->comm);
  if (c->n > 1) {
    bool live = true;
    for (uint32_t j = 0; j < c->n; j++) live = live && c->w[j].th.joinable();
    if (live) (void)synchronize_all(c, false);  // (the last batches complete on every shard together)
    stop_shards(c);
    for (uint32_t j = 0; j < c->n; j++)
      if (c->r[j]) comm_destroy(c->r[j]);
    if (c->stats_ring) (void)hipHostFree(c->stats_ring);
  }
  for (uint32_t j = 0; j < c->n; j++)
    if (c->e[j]) eng_destroy(c->e[j]);
  delete c;
}

int rl_do_limit_async(rl_ctx* c, const rl_batch* in, rl_result* out, void* stream) {
  if (!c || !in || !out) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->n == 1) return eng_do_limit_async(c->e[0], in, out, stream);
  if ((uintptr_t)in->stem_bytes & 3u) return fail(c, RL_E_INVALID, "gpu: stem_bytes must be 4-byte aligned");
  return shards_submit(c, in, out, false, (hipStream_t)stream);
}

// A host batch for the shards: the checks of the single-table path, on the
// whole batch (a batch is taken by every shard or by none).
int check_host_batch(rl_ctx* c, const rl_batch* in, const rl_result* out) {
  const uint32_t n = in->n, nq = in->n_requests;
  if (n && (!in->stem_off || !in->req_idx || !out->code || !out->limit_remaining))
    return fail(c, RL_E_INVALID, "gpu: null argument");
  const uint64_t nb = n ? in->stem_off[n] : 0;
  if (n > c->cfg.max_batch || nq > c->cfg.max_requests || in->n_rules > c->cfg.max_rules ||
      nb > c->cfg.max_stem_bytes)
    return fail(c, RL_E_CAPACITY, "gpu: batch exceeds configured max_batch/max_requests/max_rules/max_stem_bytes");
  if (n && !nq) return fail(c, RL_E_INVALID, "gpu: descriptors without requests");
  return RL_OK;
}

int rl_do_limit_host_async(rl_ctx* c, const rl_batch* in, rl_result* out) {
  if (!c || !in || !out) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->n == 1) return eng_do_limit_host_async(c->e[0], in, out);
  if (const int rc = check_host_batch(c, in, out)) return rc;
  return shards_submit(c, in, out, true, nullptr);
}

int rl_do_limit_compact_async(rl_ctx* c, const rl_batch_compact* in, rl_result* out) {
  if (!c || !in || !out) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->comm) return eng_fail(c->e[0], RL_E_INVALID, "gpu: compact batches are not routed (rl_do_limit_routed_async)");
  if (c->n == 1) return eng_do_limit_compact_async(c->e[0], in, out);
  // a multi-shard ctx: one request-aligned slice per shard, each over its own
  // device's link (rl_comm's stage_host_compact: the slice's parts, unpacked
  // on the device), then the shards' exchange as for rl_batch host batches
  // (the shards hold n x max_rules rows: check the ctx's own limit first)
  if (in->n_rules > c->cfg.max_rules) return fail(c, RL_E_CAPACITY, "gpu: batch exceeds configured max_rules");
  if (const int rc = eng_compact_check(c->e[0], in, out)) return from_engine(c, c->e[0], rc);
  const uint32_t* first = reinterpret_cast<const uint32_t*>(in->buf + in->req_first);
  if (in->n_requests && (first[0] != 0 || first[in->n_requests] != in->n))
    return fail(c, RL_E_INVALID, "gpu: compact batch request layout is not a partition of the descriptors");
  rl_batch sizes{};
  sizes.n = in->n;
  sizes.n_requests = in->n_requests;
  sizes.n_rules = in->n_rules;
  return shards_submit(c, &sizes, out, true, nullptr, in);
}

int rl_batch_progress(rl_ctx* c, uint64_t* submitted, uint64_t* completed) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->n > 1 || c->comm) return fail(c, RL_E_INVALID, "gpu: rl_batch_progress is for single-shard ctxs");
  return eng_batch_progress(c->e[0], submitted, completed);
}

int rl_do_limit_prefixed_async(rl_ctx* c, const rl_batch_prefixed* in, rl_result* out) {
  if (!c || !in || !out) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->comm) {
    // a ctx that joined a communicator (one process per GPU): the whole
    // prefix-shared batch is this rank's slice of the node batch, staged over
    // this GPU's link and unpacked on it, then routed like a device slice
    // (collective, as rl_do_limit_routed_async; out->stats = this rank's
    // requests' deltas). The Go batcher of every rank submits one batch per
    // tick, empty when idle.
    uint32_t tiles = 0;
    if (const int rc = eng_prefixed_check(c->e[0], in, out, &tiles)) {
      // a rejected slice still takes part in the exchange (no records) and
      // fails at rl_synchronize: no peer waits for it
      rl_batch none{};
      rl_result nout = *out;
      return comm_do_limit(c->comm, c->e[0], &none, &nout, nullptr, nullptr, rc);  // (RL_OK unless the router broke)
    }
    rl_batch sizes{};
    sizes.n = in->n;
    sizes.n_requests = in->n_requests;
    sizes.n_rules = in->n_rules;
    CommIO io;
    io.host = true;
    io.pb = in;
    io.t0 = 0;
    io.t1 = tiles;
    io.stats_host = in->n_rules ? (unsigned long long*)out->stats : nullptr;
    return comm_do_limit(c->comm, c->e[0], &sizes, out, nullptr, &io);
  }
  if (c->n == 1) return eng_do_limit_prefixed_async(c->e[0], in, out);
  // a multi-shard ctx: one slice of request tiles per shard, each over its own
  // device's link (rl_comm's stage_host_prefixed), then the shards' exchange
  uint32_t tiles = 0;
  if (in->n_rules > c->cfg.max_rules) return fail(c, RL_E_CAPACITY, "gpu: batch exceeds configured max_rules");
  if (const int rc = eng_prefixed_check(c->e[0], in, out, &tiles)) return from_engine(c, c->e[0], rc);
  rl_batch sizes{};
  sizes.n = in->n;
  sizes.n_requests = in->n_requests;
  sizes.n_rules = in->n_rules;
  return shards_submit(c, &sizes, out, true, nullptr, nullptr, in);
}

int rl_do_limit(rl_ctx* c, const rl_batch* in, rl_result* out) {
  if (!c || !in || !out) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->n == 1) return eng_do_limit(c->e[0], in, out);
  if (const int rc = check_host_batch(c, in, out)) return rc;
  const int rc = shards_submit(c, in, out, true, nullptr);
  const int sr = synchronize_all(c);
  return rc ? rc : sr;
}

int rl_comm_unique_id(uint8_t* id) {
  if (!id) return fail(nullptr, RL_E_INVALID, "gpu: null argument");
  std::string err;
  const int rc = comm_unique_id(id, &err);
  if (rc) return fail(nullptr, rc, err);
  return RL_OK;
}

int rl_comm_loopback_id(uint8_t* id) {
  if (!id) return fail(nullptr, RL_E_INVALID, "gpu: null argument");
  std::string err;
  const int rc = comm_loopback_id(id, &err);
  if (rc) return fail(nullptr, rc, err);
  return RL_OK;
}

int rl_comm_init(rl_ctx* c, uint32_t world, uint32_t rank, const uint8_t* id) {
  if (!c || !id) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->n > 1) return fail(c, RL_E_INVALID, "gpu: rl_comm_init needs a single-shard ctx (one per process and GPU)");
  if (c->comm) return eng_fail(c->e[0], RL_E_INVALID, "gpu: ctx already joined a communicator");
  if (!c->cfg.hash_seed)
    return eng_fail(c->e[0], RL_E_INVALID, "gpu: a routed table needs an explicit hash_seed shared by every rank");
  std::string err;
  c->comm = comm_create(c->e[0], world, rank, id, &err);
  if (!c->comm) return eng_fail(c->e[0], RL_E_COMM, err);
  return RL_OK;
}

int rl_do_limit_routed_async(rl_ctx* c, const rl_batch* in, rl_result* out, void* stream) {
  if (!c || !in || !out) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (!c->comm) return fail(c, RL_E_INVALID, "gpu: ctx has no communicator (rl_comm_init)");
  return comm_do_limit(c->comm, c->e[0], in, out, (hipStream_t)stream);
}

int rl_synchronize(rl_ctx* c) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  return synchronize_all(c);
}

int rl_sweep(rl_ctx* c, int64_t now, uint64_t* n_evicted) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  int rc = settle(c);
  if (rc) return rc;
  if (c->comm) {  // (routed: one floor for the world, the least of the ranks' now)
    rc = from_engine(c, c->e[0], comm_sweep_floor(c->comm, c->e[0], now, &now));
    if (rc) return rc;
  }
  uint64_t total = 0;
  for (uint32_t j = 0; j < c->n; j++) {
    uint64_t ev = 0;
    rc = from_engine(c, c->e[j], eng_sweep(c->e[j], now, &ev));
    if (rc) return rc;
    total += ev;
  }
  if (n_evicted) *n_evicted = total;
  return RL_OK;
}

int rl_restore(rl_ctx* c, const rl_restore_batch* r) {
  if (!c || !r) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (const int src = settle(c)) return src;
  if (c->n == 1) return eng_restore(c->e[0], r);
  // route the SET records by owner on the host (restores are rare)
  std::vector<rlsplit::Sub> part;
  if (!split_by_owner(c, r->n, r->stem_bytes, r->stem_off, &part)) return fail(c, RL_E_INVALID, "gpu: restore stem offsets");
  for (uint32_t j = 0; j < c->n; j++) {
    const rlsplit::Sub& s = part[j];
    if (s.idx.empty()) continue;
    const auto unit = rlsplit::take(r->unit, s.idx), lc = rlsplit::take(r->lc, s.idx);
    const auto now = rlsplit::take(r->now, s.idx);
    const auto count = rlsplit::take(r->count, s.idx);
    const rl_restore_batch sub{(uint32_t)s.idx.size(), 0,          s.stems.data(), s.off.data(),
                               unit.data(),            now.data(), count.data(),   lc.data()};
    const int rc = from_engine(c, c->e[j], eng_restore(c->e[j], &sub));
    if (rc) return rc;
  }
  return RL_OK;
}

int rl_table_info_get(rl_ctx* c, rl_table_info* info) {
  if (!c || !info) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (const int src = settle_local(c)) return src;
  rl_table_info sum{};
  for (uint32_t j = 0; j < c->n; j++) {
    rl_table_info x{};
    const int rc = from_engine(c, c->e[j], eng_table_info_get(c->e[j], &x));
    if (rc) return rc;
    sum.table_slots += x.table_slots;
    sum.live_slots += x.live_slots;
    sum.tombstones += x.tombstones;
    sum.arena_bytes_used += x.arena_bytes_used;
    sum.exact_stems += x.exact_stems;
    sum.decisions += x.decisions;
    sum.history_entries += x.history_entries;
    sum.history_appended += x.history_appended;
    sum.history_lost += x.history_lost;
    sum.history_slots += x.history_slots;
    sum.history_refused += x.history_refused;
    sum.batches = std::max(sum.batches, x.batches);
  }
  *info = sum;
  return RL_OK;
}

int rl_local_cache_info_get(rl_ctx* c, int64_t now, rl_local_cache_info* info) {
  if (!c || !info) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (const int src = settle_local(c)) return src;
  rl_local_cache_info sum{};
  for (uint32_t j = 0; j < c->n; j++) {
    rl_local_cache_info x{};
    const int rc = from_engine(c, c->e[j], eng_local_cache_info_get(c->e[j], now, &x));
    if (rc) return rc;
    sum.entry_count += x.entry_count;
    sum.lookup_count += x.lookup_count;
    sum.hit_count += x.hit_count;
    sum.miss_count += x.miss_count;
  }
  *info = sum;
  return RL_OK;
}

int rl_snapshot_size(rl_ctx* c, uint64_t* bytes) {
  if (!c || !bytes) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->n == 1) return eng_snapshot_size(c->e[0], bytes);
  uint64_t total = 8 * (2 + c->n);  // magic, n, per-shard sizes
  for (uint32_t j = 0; j < c->n; j++) {
    uint64_t b = 0;
    const int rc = from_engine(c, c->e[j], eng_snapshot_size(c->e[j], &b));
    if (rc) return rc;
    total += b;
  }
  *bytes = total;
  return RL_OK;
}

int rl_snapshot_save(rl_ctx* c, void* host, uint64_t bytes) {
  if (!c || !host) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (const int src = settle(c)) return src;
  if (c->n == 1) return eng_snapshot_save(c->e[0], host, bytes);
  uint64_t* h = (uint64_t*)host;
  const uint64_t head = 8 * (2 + c->n);
  if (bytes < head) return fail(c, RL_E_CAPACITY, "gpu: snapshot buffer smaller than rl_snapshot_size");
  h[0] = MSNAP_MAGIC;
  h[1] = c->n;
  uint64_t pos = head;
  for (uint32_t j = 0; j < c->n; j++) {
    uint64_t b = 0;
    int rc = from_engine(c, c->e[j], eng_snapshot_size(c->e[j], &b));
    if (rc) return rc;
    if (pos + b > bytes) return fail(c, RL_E_CAPACITY, "gpu: snapshot buffer smaller than rl_snapshot_size");
    rc = from_engine(c, c->e[j], eng_snapshot_save(c->e[j], (uint8_t*)host + pos, b));
    if (rc) return rc;
    h[2 + j] = b;
    pos += b;
  }
  return RL_OK;
}

int rl_snapshot_load(rl_ctx* c, const void* host, uint64_t bytes) {
  if (!c || !host) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (const int src = settle(c)) return src;
  if (c->n == 1) return eng_snapshot_load(c->e[0], host, bytes);
  const uint64_t* h = (const uint64_t*)host;
  if (bytes < 16 || h[0] != MSNAP_MAGIC || h[1] != c->n || bytes < 8 * (2 + c->n))
    return fail(c, RL_E_INVALID, "gpu: not a snapshot of a ctx with this many shards");
  uint64_t pos = 8 * (2 + c->n);
  for (uint32_t j = 0; j < c->n; j++) {
    if (pos + h[2 + j] > bytes) return fail(c, RL_E_INVALID, "gpu: snapshot truncated");
    const int rc = from_engine(c, c->e[j], eng_snapshot_load(c->e[j], (const uint8_t*)host + pos, h[2 + j]));
    if (rc) return rc;
    pos += h[2 + j];
  }
  return RL_OK;
}

int rl_export_range(rl_ctx* c, uint32_t shard, uint64_t slot_begin, uint64_t slot_end, rl_records* out,
                    rl_export_info* info) {
  if (!c || !info) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->comm) return fail(c, RL_E_INVALID, "gpu: rl_export_range is not for a ctx that joined a communicator");
  if (shard >= c->n) return fail(c, RL_E_INVALID, "gpu: bad shard");
  if (const int src = settle_local(c)) return src;
  return from_engine(c, c->e[shard], eng_export_range(c->e[shard], slot_begin, slot_end, out, info));
}

int rl_resize(rl_ctx* c, uint64_t table_slots, rl_resize_info* info) {
  if (const int rc = resize_refused(c, "rl_resize")) return rc;
  if (const int rc = from_engine(c, c->e[0], eng_resize_check(c->e[0], table_slots))) return rc;
  if (const int src = settle_local(c)) return src;
  for (uint32_t j = 0; j < c->n; j++) c->w[j].rs_slots = table_slots;
  rl_resize_info sum{};
  const int placed = c->n == 1 ? eng_resize_place(c->e[0], table_slots, &c->w[0].rs_plan)  // (no workers: here)
                               : run_shards(c, ShardWorker::RESIZE);
  const int rc = resize_commit_all(
      c, placed, [&](uint32_t j) { return &c->w[j].rs_plan; },
      [&](Engine* e, ResizePlan* p) {
        const int rc = eng_resize_commit(e, p);
        const rl_resize_info& x = p->info;
        sum.slots_before += x.slots_before;
        sum.slots_after += x.slots_after;
        sum.keys += x.keys;
        sum.tombstones_dropped += x.tombstones_dropped;
        sum.log_entries_relinked += x.log_entries_relinked;
        sum.longest_probe = std::max(sum.longest_probe, x.longest_probe);
        return rc;
      });
  if (rc) return rc;
  c->cfg.table_slots = table_slots;
  if (info) *info = sum;
  return RL_OK;
}

int rl_resize_history(rl_ctx* c, uint64_t history_entries, rl_history_resize_info* info) {
  if (const int rc = resize_refused(c, "rl_resize_history")) return rc;
  if (const int rc = from_engine(c, c->e[0], eng_relog_check(c->e[0], history_entries))) return rc;
  if (const int src = settle_local(c)) return src;
  for (uint32_t j = 0; j < c->n; j++) c->w[j].rl_entries = history_entries;
  rl_history_resize_info sum{};
  const int placed = c->n == 1 ? eng_relog_place(c->e[0], history_entries, &c->w[0].rl_plan)  // (no workers: here)
                               : run_shards(c, ShardWorker::RELOG);
  const int rc = resize_commit_all(
      c, placed, [&](uint32_t j) { return &c->w[j].rl_plan; },
      [&](Engine* e, RelogPlan* p) {
        const int rc = eng_relog_commit(e, p);
        const rl_history_resize_info& x = p->info;
        sum.entries_before += x.entries_before;
        sum.entries_after += x.entries_after;
        sum.written_before += x.written_before;
        sum.entries_kept += x.entries_kept;
        sum.entries_dropped += x.entries_dropped;
        sum.chains += x.chains;
        sum.chains_lost += x.chains_lost;
        sum.fill_max = std::max(sum.fill_max, x.fill_max);
        sum.longest_chain = std::max(sum.longest_chain, x.longest_chain);
        return rc;
      });
  if (rc) return rc;
  c->cfg.history_entries = c->e[0]->cfg.history_entries;
  if (info) *info = sum;
  return RL_OK;
}

int rl_resize_arena(rl_ctx* c, uint64_t arena_bytes) {
  if (const int rc = resize_refused(c, "rl_resize_arena")) return rc;
  if (const int rc = from_engine(c, c->e[0], eng_arena_check(c->e[0], arena_bytes))) return rc;
  if (const int src = settle_local(c)) return src;
  ArenaPlan plan[MAX_LOCAL_SHARDS];
  int rc = RL_OK;
  for (uint32_t j = 0; j < c->n && !rc; j++) rc = from_engine(c, c->e[j], eng_arena_place(c->e[j], arena_bytes, &plan[j]));
  rc = resize_commit_all(
      c, rc, [&](uint32_t j) { return &plan[j]; },
      [](Engine* e, ArenaPlan* p) {
        eng_arena_commit(e, p);
        return (int)RL_OK;
      });
  if (rc) return rc;
  c->cfg.arena_bytes = arena_bytes;
  return RL_OK;
}

int rl_import(rl_ctx* c, const rl_records* in) {
  if (!c || !in) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->comm) return fail(c, RL_E_INVALID, "gpu: rl_import is not for a ctx that joined a communicator");
  if (const int src = settle_local(c)) return src;
  if (c->n == 1) return eng_import(c->e[0], in);
  // the whole call is checked first (a bad record leaves every shard untouched),
  // then the records go to their owners, routed on the host like rl_restore's
  if (const int rc = from_engine(c, c->e[0], eng_import_check(c->e[0], in))) return rc;
  std::vector<rlsplit::Sub> part;
  split_by_owner(c, in->n, in->stem_bytes, in->stem_off, &part);
  for (uint32_t j = 0; j < c->n; j++) {
    rlsplit::Sub& s = part[j];
    if (s.idx.empty()) continue;
    auto unit = rlsplit::take(in->unit, s.idx), flags = rlsplit::take(in->flags, s.idx);
    auto ws = rlsplit::take(in->ws, s.idx), count = rlsplit::take(in->count, s.idx);
    auto expire = rlsplit::take(in->expire, s.idx), lc = rlsplit::take(in->lc, s.idx);
    const rl_records sub{(uint32_t)s.idx.size(), 0,         0,            s.stems.data(), s.off.data(), unit.data(),
                         flags.data(),           ws.data(), count.data(), expire.data(),  lc.data()};
    const int rc = from_engine(c, c->e[j], eng_import(c->e[j], &sub));
    if (rc) return rc;
  }
  return RL_OK;
}

int rl_lookup(rl_ctx* c, const rl_keys* in, rl_key_state* out) {
  if (!c || !in || !out) return fail(c, RL_E_INVALID, "gpu: null argument");
  if (c->comm) return fail(c, RL_E_INVALID, "gpu: rl_lookup is not for a ctx that joined a communicator");
  if (const int src = settle_local(c)) return src;
  if (c->n == 1) return eng_lookup(c->e[0], in, out);
  // the whole call is checked first (a bad call writes nothing), then the keys
  // go to their owners, routed on the host like rl_import's records, and the
  // answers come back in the caller's order
  if (const int rc = from_engine(c, c->e[0], eng_lookup_check(c->e[0], in, out))) return rc;
  std::vector<rlsplit::Sub> part;
  split_by_owner(c, in->n, in->stem_bytes, in->stem_off, &part);
  // (the shards' answers lie one after the other in arrays of the call's size)
  std::vector<uint8_t> status(in->n), found(in->n);
  std::vector<uint32_t> count(in->n), expire(in->n), lc(in->n);
  size_t at = 0;
  for (uint32_t j = 0; j < c->n; at += part[j++].idx.size()) {
    rlsplit::Sub& s = part[j];
    if (s.idx.empty()) continue;
    const auto unit = rlsplit::take(in->unit, s.idx);
    const auto now = rlsplit::take(in->now, s.idx);
    s.stems.push_back(0);  // (never null, even when every stem is empty)
    const rl_keys k{(uint32_t)s.idx.size(), 0, s.stems.data(), s.off.data(), unit.data(), now.data()};
    rl_key_state o{status.data() + at, found.data() + at, count.data() + at, expire.data() + at, lc.data() + at};
    if (const int rc = from_engine(c, c->e[j], eng_lookup(c->e[j], &k, &o))) return rc;  // (nothing scattered yet)
  }
  at = 0;
  for (uint32_t j = 0; j < c->n; at += part[j++].idx.size()) {
    rlsplit::put(out->status, part[j].idx, status.data() + at);
    rlsplit::put(out->found, part[j].idx, found.data() + at);
    rlsplit::put(out->count, part[j].idx, count.data() + at);
    rlsplit::put(out->expire, part[j].idx, expire.data() + at);
    rlsplit::put(out->lc, part[j].idx, lc.data() + at);
  }
  return RL_OK;
}

int rl_forget(rl_ctx* c, const rl_stems* in, uint32_t* removed, rl_forget_info* info) {
  if (!c || !in) return fail_call(c, RL_E_INVALID, "gpu: null argument");
  if (c->comm) return fail_call(c, RL_E_INVALID, "gpu: rl_forget is not for a ctx that joined a communicator");
  if (c->n == 1) return eng_forget(c->e[0], in, removed, info);
  // the whole call is checked first: a bad call changes no shard
  if (const int rc = from_engine(c, c->e[0], eng_forget_check(c->e[0], in))) return rc;
  if (const int src = settle_local(c)) return src;
  const uint32_t N = c->n;
  rl_forget_info sum{};
  if (!in->n) {
    if (info) *info = sum;
    return RL_OK;
  }
  auto add = [&](const rl_forget_info& x) {
    sum.slots_scanned += x.slots_scanned;
    sum.keys += x.keys;
    sum.keys_with_history += x.keys_with_history;
    sum.arena_bytes += x.arena_bytes;
  };
  if (in->flags & RL_FORGET_PREFIX) {
    // every shard scans its own table on its own device and worker, for all the prefixes
    for (uint32_t j = 0; j < N; j++) c->w[j].fg_in = in;
    if (const int rc = run_shards(c, ShardWorker::FORGET)) return rc;
    for (uint32_t j = 0; j < N; j++) add(c->w[j].fg_info);
    if (removed)
      for (uint32_t i = 0; i < in->n; i++) {
        removed[i] = 0;
        for (uint32_t j = 0; j < N; j++) removed[i] += c->w[j].fg_removed[i];
      }
    if (info) *info = sum;
    return RL_OK;
  }
  // keyed stems go to their owners, routed on the host like rl_lookup's keys,
  // and the counts come back in the caller's order
  std::vector<rlsplit::Sub> part;
  split_by_owner(c, in->n, in->stem_bytes, in->stem_off, &part);
  std::vector<std::vector<uint32_t>> got(N);
  for (uint32_t j = 0; j < N; j++) {
    const rlsplit::Sub& s = part[j];
    if (s.idx.empty()) continue;
    got[j].resize(s.idx.size());
    const rl_stems sub{(uint32_t)s.idx.size(), in->flags, s.stems.data(), s.off.data()};
    rl_forget_info x{};
    if (const int rc = from_engine(c, c->e[j], eng_forget(c->e[j], &sub, got[j].data(), &x))) return rc;
    add(x);
  }
  if (removed)
    for (uint32_t j = 0; j < N; j++) rlsplit::put(removed, part[j].idx, got[j].data());
  if (info) *info = sum;
  return RL_OK;
}

int rl_scan(rl_ctx* c, const rl_scan_query* q, rl_scan_cursor* cur, rl_records* out, rl_scan_prefix_sum* by_prefix,
            rl_scan_info* info) {
  if (!c || !q || !cur) return fail_call(c, RL_E_INVALID, "gpu: null argument");
  if (c->comm) return fail_call(c, RL_E_INVALID, "gpu: rl_scan is not for a ctx that joined a communicator");
  if (cur->reserved) return fail_call(c, RL_E_INVALID, "gpu: rl_scan: cursor's reserved field not zero");
  if (cur->shard > c->n) return fail_call(c, RL_E_INVALID, "gpu: rl_scan: cursor shard beyond n_shards");
  // the whole call is checked first: a failed call writes nothing
  if (const int rc = from_engine(c, c->e[0], eng_scan_check(c->e[0], q, out))) return rc;
  if (cur->shard == c->n) {  // the scan is complete: the empty answer
    if (cur->slot) return fail_call(c, RL_E_INVALID, "gpu: rl_scan: a finished cursor's slot is 0");
    if (out) {
      out->n = 0;
      out->stem_off[0] = 0;
    }
    if (by_prefix)
      for (uint32_t p = 0; p < std::max(q->n_prefixes, 1u); p++) by_prefix[p] = rl_scan_prefix_sum{};
    if (info) *info = rl_scan_info{};
    return RL_OK;
  }
  if (const int src = settle_local(c)) return src;
  Engine* e = c->e[cur->shard];
  uint64_t slot = cur->slot;
  if (const int rc = from_engine(c, e, eng_scan(e, q, &slot, out, by_prefix, info))) return rc;
  if (slot >= e->nslots) {
    cur->shard += 1;
    cur->slot = 0;
  } else {
    cur->slot = slot;
  }
  return RL_OK;
}

int rl_hot_keys(rl_ctx* c, const rl_hot_query* q, rl_records* out, rl_hot_info* info) {
  if (!c || !q || !info) return fail_call(c, RL_E_INVALID, "gpu: null argument");
  if (c->comm) return fail_call(c, RL_E_INVALID, "gpu: rl_hot_keys is not for a ctx that joined a communicator");
  // the whole call is checked first: a failed call writes nothing
  if (q->k && (!out || !records_check(out, true)))
    return fail_call(c, RL_E_INVALID, "gpu: rl_hot_keys: null rl_records (or one of its arrays) with k > 0");
  for (uint32_t j = 0; j < c->n; j++)
    if (const int rc = from_engine(c, c->e[j], eng_hot_check(c->e[j], q))) return rc;
  if (const int src = settle_local(c)) return src;
  // every shard's own top k on its own device, merged on the host: the top k
  // of the union is the top k
  std::vector<HotAnswer> ans(c->n);
  std::vector<std::vector<rlhot::Rec>> part(c->n);
  rl_hot_info sum{};
  for (uint32_t j = 0; j < c->n; j++) {
    rl_hot_info x{};
    if (const int rc = from_engine(c, c->e[j], eng_hot_keys(c->e[j], q, &ans[j], &x))) return rc;
    sum.slots += x.slots;
    sum.matched += x.matched;
    sum.hits += x.hits;
    sum.time_floor = j ? std::max(sum.time_floor, x.time_floor) : x.time_floor;
    const HotAnswer& a = ans[j];
    for (size_t i = 0; i < a.count.size(); i++)
      part[j].push_back(rlhot::Rec{a.count[i], a.ws[i], a.expire[i], a.lc[i], a.unit[i], a.len[i], a.stem.data() + a.off[i]});
  }
  const std::vector<rlhot::Rec> top = rlhot::merge(part, q->k);
  rlhot::summarize(top, &sum.threshold, &sum.above);
  uint64_t nb = 0;
  for (const rlhot::Rec& r : top) nb += r.len;
  *info = sum;
  if (!out) return RL_OK;
  if (top.size() > out->n || nb > out->stem_cap || nb > 0xFFFFFFFFull)
    return fail_call(c, RL_E_CAPACITY, "gpu: rl_hot_keys: the answer holds " + std::to_string(top.size()) + " records / " +
                                           std::to_string(nb) + " stem bytes: larger than rl_records");
  out->n = (uint32_t)top.size();
  if (out->stem_off) out->stem_off[0] = 0;
  uint32_t at = 0;
  for (size_t i = 0; i < top.size(); i++) {
    const rlhot::Rec& r = top[i];
    memcpy(out->stem_bytes + at, r.stem, r.len);
    at += r.len;
    out->stem_off[i + 1] = at;
    out->unit[i] = (uint8_t)r.unit;
    out->flags[i] = 0;
    out->ws[i] = r.ws;
    out->count[i] = r.count;
    out->expire[i] = r.expire;
    out->lc[i] = r.lc;
  }
  return RL_OK;
}

int rl_config_load(rl_ctx* c, const rl_config_tree* t) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  if (c->n > 1 && t && t->nodes)  // (the shards' own check allows their n x max_rules rows)
    for (uint32_t i = 0; i < t->n_nodes; i++)
      if (t->nodes[i].rule_id >= c->cfg.max_rules)
        return fail(c, RL_E_INVALID, "gpu: config node " + std::to_string(i) + ": rule id >= max_rules");
  for (uint32_t j = 0; j < c->n; j++) {
    const int rc = from_engine(c, c->e[j], eng_config_load(c->e[j], t));
    if (rc) return rc;
  }
  return RL_OK;
}

// rl_do_limit_requests, with the per-request verdict when asked for.
static int do_limit_requests(rl_ctx* c, const rl_request_batch* in, rl_request_result* out, uint32_t opts,
                             rl_request_verdict* verdict) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  if (c->comm) return fail(c, RL_E_INVALID, "gpu: rl_do_limit_requests is not routed (rl_do_limit_routed_async)");
  if (c->n == 1) return eng_do_limit_requests(c->e[0], in, out, nullptr, nullptr, opts, verdict);
  // a multi-shard ctx: the config match on shard 0's GPU, the matched batch
  // through the shards as a device batch (shard 0 partitions it, every owner
  // answers its keys), then the expansion to the request layout on shard 0
  int rc = synchronize_all(c);  // (earlier batches first: the call is synchronous)
  if (rc) return rc;
  struct Run {
    rl_ctx* c;
    bool failed;
  } u{c, false};
  auto run = [](void* p, const rl_batch* din, rl_result* dout, hipStream_t st) -> int {
    Run& r = *static_cast<Run*>(p);
    const int sr = shards_submit(r.c, din, dout, false, st);
    const int yr = synchronize_all(r.c);
    r.failed = sr || yr;
    return sr ? sr : yr;
  };
  rc = eng_do_limit_requests(c->e[0], in, out, run, &u, opts, verdict);
  return u.failed ? rc : from_engine(c, c->e[0], rc);
}

int rl_do_limit_requests(rl_ctx* c, const rl_request_batch* in, rl_request_result* out) {
  return do_limit_requests(c, in, out, 0, nullptr);
}

int rl_do_limit_requests_verdict(rl_ctx* c, const rl_request_batch* in, rl_request_result* out, uint32_t opts,
                                 rl_request_verdict* verdict) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  if (!verdict) return fail(c, RL_E_INVALID, "gpu: null rl_request_verdict");
  return do_limit_requests(c, in, out, opts, verdict);
}

int rl_do_limit_requests_packed_async(rl_ctx* c, const rl_request_batch_packed* in, rl_request_result* out,
                                      uint32_t opts, rl_request_verdict* verdict) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  const char* single = "gpu: rl_do_limit_requests_packed_async is for single-shard ctxs (use rl_do_limit_requests_verdict)";
  if (c->n > 1) return fail(c, RL_E_INVALID, single);
  if (c->comm) return eng_fail(c->e[0], RL_E_INVALID, single);
  return eng_do_limit_requests_packed_async(c->e[0], in, out, opts, verdict);
}

int rl_do_limit_wire_async(rl_ctx* c, const rl_wire_batch* in, rl_wire_result* wire, rl_request_result* out,
                           uint32_t opts, rl_request_verdict* verdict) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  const char* single = "gpu: rl_do_limit_wire_async is for single-shard ctxs";
  if (c->n > 1) return fail(c, RL_E_INVALID, single);
  if (c->comm) return eng_fail(c->e[0], RL_E_INVALID, single);
  return eng_do_limit_wire_async(c->e[0], in, wire, out, opts, verdict);
}

int rl_do_limit_wire_respond_async(rl_ctx* c, const rl_wire_batch* in, rl_wire_result* wire, rl_request_result* out,
                                   uint32_t opts, rl_request_verdict* verdict, const rl_response_format* fmt,
                                   rl_response_batch* resp) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  const char* single = "gpu: rl_do_limit_wire_respond_async is for single-shard ctxs";
  if (c->n > 1) return fail(c, RL_E_INVALID, single);
  if (c->comm) return eng_fail(c->e[0], RL_E_INVALID, single);
  if (!resp) return eng_fail(c->e[0], RL_E_INVALID, "gpu: null rl_response_batch");
  return eng_do_limit_wire_async(c->e[0], in, wire, out, opts, verdict, fmt, resp);
}

int rl_override_rules_enable(rl_ctx* c, const rl_override_rules_config* cfg) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  const char* single = "gpu: rl_override_rules_enable is for single-shard ctxs (the wire paths')";
  if (c->n > 1) return fail(c, RL_E_INVALID, single);
  if (c->comm) return eng_fail(c->e[0], RL_E_INVALID, single);
  return eng_override_rules_enable(c->e[0], cfg);
}

int rl_override_rules_info_get(rl_ctx* c, rl_override_rules_info* info) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  if (c->n > 1) return fail(c, RL_E_INVALID, "gpu: override rules are not enabled on this ctx (rl_override_rules_enable)");
  return eng_override_rules_info_get(c->e[0], info);
}

int rl_override_rule_keys(rl_ctx* c, uint32_t from_rule, uint32_t n, uint8_t* bytes, uint64_t cap, uint32_t* off,
                          uint64_t* needed) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  if (c->n > 1) return fail(c, RL_E_INVALID, "gpu: override rules are not enabled on this ctx (rl_override_rules_enable)");
  return eng_override_rule_keys(c->e[0], from_rule, n, bytes, cap, off, needed);
}

int rl_debug_respond(rl_ctx* c, uint32_t n_requests, uint32_t n_descriptors, const uint32_t* req_idx,
                     const uint8_t* req_status, const rl_request_result* answers, uint32_t opts,
                     const rl_response_format* fmt, rl_response_batch* resp) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  return from_engine(c, c->e[0], eng_debug_respond(c->e[0], n_requests, n_descriptors, req_idx, req_status, answers,
                                                    opts, fmt, resp));
}

int rl_debug_verdict(rl_ctx* c, uint32_t n_requests, uint32_t n_descriptors, const uint32_t* req_idx,
                     const uint8_t* match, const uint8_t* code, const uint32_t* limit_remaining,
                     const uint32_t* reset_s, const uint32_t* requests_per_unit, uint32_t opts,
                     rl_request_verdict* verdict) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  return from_engine(c, c->e[0], eng_debug_verdict(c->e[0], n_requests, n_descriptors, req_idx, match, code,
                                                    limit_remaining, reset_s, requests_per_unit, opts, verdict));
}

// Diagnostics, profiling and the per-rank routing halves act on shard 0.
int rl_table_info_shard(rl_ctx* c, uint32_t shard, rl_table_info* info) {
  if (!c || !info || shard >= c->n) return fail(c, RL_E_INVALID, "gpu: bad shard");
  return from_engine(c, c->e[shard], eng_table_info_get(c->e[shard], info));
}

int rl_debug_keys(rl_ctx* c, const rl_batch* in, uint8_t* out_bytes, uint32_t* out_off, uint32_t out_cap) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  return from_engine(c, c->e[0], eng_debug_keys(c->e[0], in, out_bytes, out_off, out_cap));
}

int rl_debug_log_tear(rl_ctx* c, const rl_log_tear* arm, rl_log_tear* out) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  return from_engine(c, c->e[0], eng_debug_log_tear(c->e[0], arm, out));
}

int rl_debug_decide(rl_ctx* c, uint32_t n, const uint32_t* before, const uint32_t* after, const uint8_t* lc_hit,
                    const uint32_t* hits, const uint32_t* limit, const uint8_t* unit, const uint8_t* flags,
                    const int64_t* now, uint8_t* code, uint32_t* remaining, uint32_t* reset_s,
                    uint64_t* stat_deltas, uint8_t* lc_set) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  return from_engine(c, c->e[0], eng_debug_decide(c->e[0], n, before, after, lc_hit, hits, limit, unit, flags, now,
                                                   code, remaining, reset_s, stat_deltas, lc_set));
}

int rl_profile(rl_ctx* c, int enable) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  for (uint32_t j = 0; j < c->n; j++) {
    const int rc = from_engine(c, c->e[j], eng_profile(c->e[j], enable));
    if (rc) return rc;
  }
  return RL_OK;
}

int rl_profile_read(rl_ctx* c, double* ms, uint32_t n, uint64_t* batches) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  return from_engine(c, c->e[0], eng_profile_read(c->e[0], ms, n, batches));
}

int rl_route_pack(rl_ctx* c, const rl_batch* in, uint32_t n_shards, uint32_t src_rank, void* send_rec,
                  uint8_t* send_stem, uint32_t* perm, uint64_t* counts, void* stream) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  if (c->n > 1) return fail(c, RL_E_INVALID, "gpu: per-rank routing needs a single-shard ctx");
  return eng_route_pack(c->e[0], in, n_shards, src_rank, send_rec, send_stem, perm, counts, stream);
}

int rl_route_do_limit(rl_ctx* c, uint32_t n, const void* recv_rec, const uint8_t* recv_stem, uint64_t recv_stem_bytes,
                      const uint64_t* src_stem_base, uint32_t n_shards, uint32_t n_rules, uint32_t rule_stride,
                      uint64_t* ret, uint64_t* stats, int isolate, void* stream) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  if (c->n > 1) return fail(c, RL_E_INVALID, "gpu: per-rank routing needs a single-shard ctx");
  return eng_route_do_limit(c->e[0], n, recv_rec, recv_stem, recv_stem_bytes, src_stem_base, n_shards, n_rules,
                            rule_stride, ret, stats, isolate, stream);
}

int rl_route_scatter(rl_ctx* c, uint32_t n, const uint32_t* perm, const uint64_t* ret, rl_result* out, void* stream) {
  if (!c) return fail(c, RL_E_INVALID, "gpu: null ctx");
  if (c->n > 1) return fail(c, RL_E_INVALID, "gpu: per-rank routing needs a single-shard ctx");
  return eng_route_scatter(c->e[0], n, perm, ret, out, stream);
}

void* rl_alloc_host(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
  return p;
}

void rl_free_host(void* p) {
  if (p) (void)hipHostFree(p);
}

}  // extern "C"
