/*
 * ratelimit_hip.h — C ABI of libratelimit_hip.so, the MI355X fixed-window
 * rate-limit backend.
 *
 * Drop-in boundary: this library replaces the box below
 *   limiter.RateLimitCache.DoLimit           (reference src/limiter/cache.go:11-29)
 * as implemented by
 *   redis.fixedRateLimitCacheImpl.DoLimit    (src/redis/fixed_cache_impl.go:33-113)
 *   + limiter.BaseRateLimiter                (src/limiter/base_limiter.go:45-197)
 *   + limiter.CacheKeyGenerator              (src/limiter/cache_key.go:48-80)
 *   + redis-server INCRBY/EXPIRE and the freecache local over-limit cache.
 * A Go cgo adapter packs many in-flight DoLimit calls into
 * one rl_batch and calls rl_do_limit from a single batcher goroutine.
 *
 * Plain C types only: no torch, no HIP types in any signature.
 * Threading: one rl_ctx is driven by one host thread at a time.
 * Errors: every int-returning call returns RL_OK (0) or an rl_status code and
 * records a message readable with rl_last_error(); the Go adapter turns a
 * non-zero status into panic(redis.RedisError("gpu: "+msg)), exactly the
 * reference's backend-failure convention (src/redis/driver_impl.go:60-64).
 */
#ifndef RATELIMIT_HIP_H
#define RATELIMIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Stays 8 with rl_do_limit_requests_verdict / rl_debug_verdict and
 * rl_request_verdict: they only add symbols and types; no existing struct,
 * signature or behaviour changed. */
#define RL_ABI_VERSION 8u

/* Status codes. */
enum rl_status {
  RL_OK = 0,
  RL_E_INVALID = 1,    /* malformed batch: unit out of 1..4, offsets, sizes */
  RL_E_TABLE_FULL = 2, /* the key's probe window (min(table_slots, 65536) slots from its home)
                          holds neither an empty slot nor a tombstone: raise table_slots */
  RL_E_ARENA_FULL = 3, /* long-stem overflow arena exhausted */
  RL_E_HIP = 4,        /* HIP runtime error */
  RL_E_CAPACITY = 5,   /* batch larger than rl_config.max_* */
  RL_E_TIME = 6,       /* now outside [0, 2^32 - 2*86400], before the last sweep, or
                          moved back more than 8 windows on one key. Note: the reference's
                          clock is int64 (utils.TimeSource); this backend's is 32-bit */
  RL_E_COMM = 7,       /* multi-GPU routing (RCCL) error */
  RL_E_INTERNAL = 8
};

/* pb.RateLimitResponse_RateLimit_Unit (go-control-plane v0.9.7 rls.proto). */
enum rl_unit { RL_UNIT_SECOND = 1, RL_UNIT_MINUTE = 2, RL_UNIT_HOUR = 3, RL_UNIT_DAY = 4 };
/* pb.RateLimitResponse_Code. */
enum rl_code { RL_CODE_OK = 1, RL_CODE_OVER_LIMIT = 2 };
/* rl_batch.flags bits. */
#define RL_FLAG_SHADOW 0x1u /* config.RateLimit.ShadowMode (src/config/config.go:24) */

/* Per-rule stats counters, in stats.RateLimitStats order (src/stats/manager.go:47-55). */
enum rl_stat {
  RL_STAT_TOTAL_HITS = 0,
  RL_STAT_OVER_LIMIT = 1,
  RL_STAT_NEAR_LIMIT = 2,
  RL_STAT_OVER_LIMIT_WITH_LOCAL_CACHE = 3,
  RL_STAT_WITHIN_LIMIT = 4,
  RL_STAT_SHADOW_MODE = 5,
  RL_NUM_STATS = 6
};

/* Backend configuration: the knobs NewFixedRateLimitCacheImpl receives
 * (src/redis/fixed_cache_impl.go:118-125, src/settings/settings.go:45-50)
 * plus capacity sizing for HBM. */
typedef struct rl_config {
  uint64_t table_slots;      /* 64-B slots in the HBM table (power of 2; 0 = default 2^24) */
  uint64_t arena_bytes;      /* overflow arena for stems longer than 36 B (0 = default 64 MiB) */
  uint32_t max_batch;        /* max descriptors per rl_do_limit call (0 = default 1<<20) */
  uint32_t max_requests;     /* max requests per call (0 = max_batch) */
  uint32_t max_rules;        /* max distinct rule ids per call (0 = default 65536) */
  uint32_t max_stem_bytes;   /* max total stem bytes per call (0 = 128 * max_batch) */
  float near_limit_ratio;    /* NEAR_LIMIT_RATIO (float32, settings.go:48) */
  int32_t local_cache_enabled;  /* LOCAL_CACHE_SIZE_IN_BYTES != 0 (runner.go:95-98) */
  int32_t per_second_split;     /* REDIS_PERSECOND: SECOND-unit keys in a separate store */
  int32_t device;               /* HIP device ordinal */
  int64_t expiration_jitter_max_seconds; /* EXPIRATION_JITTER_MAX_SECONDS (>= 0): the backend fixes
                                            the draw at 0 and keeps a key's older
                                            windows for div + this many seconds (the history horizon) */
  uint64_t hash_seed;        /* key of the stem hash (SipHash-1-3); 0 = drawn at random per ctx.
                                Descriptor values are client-controlled: keep it secret. */
  uint32_t n_shards;         /* hash shards of the table held by this ctx (0 = 1); see rl_do_limit */
  uint32_t debug_hash_bits;  /* tests only: keep the top N bits of the hash's high word (0 = all 32),
                                so that many stems share one sort key and one home region;
                                33..63: keep the top N - 32 bits and set the others (sort keys
                                at the top of the range) */
  int32_t shard_device[16];  /* HIP device of shard k < n_shards (shards may share a device);
                                unused when n_shards <= 1 (cfg.device) */
  uint64_t history_entries;  /* 32-B entries of the history log holding the windows below a key's
                                newest (0 = table_slots; rounded to 64 powers of two, at least
                                max_batch / 16 each). Append-only rings: an entry overwritten while
                                a request could still ask for its window makes that request fail
                                with RL_E_TIME (counted in rl_table_info.history_lost), never a
                                wrong count */
  int32_t reserved[6];
} rl_config;

/* One packed batch (struct of arrays). Only descriptors whose limit is
 * non-nil are packed (nil limits -> {OK, nil, 0} host-side,
 * base_limiter.go:78-81); unlimited rules are nil by then (ratelimit.go:140-143).
 * Descriptors appear in arrival order: request-major, descriptor order inside
 * the request; req_idx is non-decreasing. now[] may move backwards (the
 * reference's tests do, on different keys); per (stem, unit) the table keeps
 * the windows below the newest one written while a request could still ask
 * for them (Redis keeps a key div + jitter seconds after its last hit,
 * fixed_cache_impl.go:71-74): a request whose clock is within div +
 * expiration_jitter_max_seconds of the key's newest window, or whose window
 * is at most 8 windows back, is answered exactly; an older one whose window
 * the key may have had gets RL_E_TIME.
 * The stem is the cache key without its window suffix:
 *   prefix ‖ domain ‖ '_' ‖ Σ(key ‖ '_' ‖ value ‖ '_')   (cache_key.go:62-71)
 * The full key is stem ‖ decimal((now/div)*div) (cache_key.go:73-74). */
typedef struct rl_batch {
  uint32_t n;            /* descriptors */
  uint32_t n_requests;   /* requests (length of now[]) */
  uint32_t n_rules;      /* rule ids are < n_rules (length of stats / RL_NUM_STATS) */
  uint32_t reserved;
  const uint8_t* stem_bytes;  /* concatenated stems */
  const uint32_t* stem_off;   /* n+1 offsets into stem_bytes, stem_off[0] == 0 */
  const int64_t* now;         /* [n_requests] UnixNow() of each request (seconds). The reference's
                                 clock is int64; here it must lie in [0, 2^32 - 172800] (the table
                                 stores 32-bit times) and not before the last rl_sweep: else RL_E_TIME */
  const uint32_t* req_idx;    /* [n] request of each descriptor */
  const uint8_t* unit;        /* [n] rl_unit of the descriptor's limit */
  const uint8_t* flags;       /* [n] RL_FLAG_* */
  const uint32_t* limit;      /* [n] RequestsPerUnit */
  const uint32_t* hits;       /* [n] request.HitsAddend (max(1, h) applied by the backend) */
  const uint32_t* rule_id;    /* [n] dense id of limit.Stats.Key */
} rl_batch;

/* Results, same order as the batch. stats holds THIS call's deltas
 * (n_rules x RL_NUM_STATS, row-major, overwritten); the adapter adds them to the
 * gostats counters. CurrentLimit is re-attached host-side (= limits[i].Limit). */
typedef struct rl_result {
  uint8_t* code;              /* [n] rl_code */
  uint32_t* limit_remaining;  /* [n] LimitRemaining */
  uint32_t* reset_s;          /* [n] DurationUntilReset.Seconds (1..86400). May be NULL on the
                                 host-buffer entry points (rl_do_limit, rl_do_limit_host_async,
                                 _compact_async, _prefixed_async): not copied back, 4 B per decision less over PCIe;
                                 the caller computes it as utils.CalculateReset does
                                 (utilities.go:32-36: div - now % div, now the request's clock) */
  uint64_t* stats;            /* [n_rules * RL_NUM_STATS] */
  uint8_t* status;            /* [n] or NULL. Non-NULL: per-descriptor failure isolation. A
                                 descriptor that cannot be answered (bad unit / rule id / stem length:
                                 RL_E_INVALID; clock: RL_E_TIME; no slot: RL_E_TABLE_FULL /
                                 RL_E_ARENA_FULL) gets that rl_status here, code 0 and no stats; the
                                 rest of the batch is answered and the call returns RL_OK. The adapter
                                 fails only the RPCs holding a failed descriptor, as the reference's
                                 per-call checkError does (fixed_cache_impl.go:90-95,
                                 ratelimit.go:252-256). NULL: any such failure fails the whole call
                                 (and the batch leaves the table untouched). A malformed batch
                                 layout (offsets, request order) always fails the call. */
} rl_result;

/* Table restore / seed records: set the fixed-window counter of key
 * stem ‖ decimal(ws(now[i], unit[i])) to count[i] with EXPIRE div (as if the last
 * INCRBY happened at now[i]); lc[i] != 0 also inserts the key into the local
 * over-limit cache with TTL div. Host memory. */
typedef struct rl_restore_batch {
  uint32_t n;
  uint32_t reserved;
  const uint8_t* stem_bytes;
  const uint32_t* stem_off;   /* n+1 */
  const uint8_t* unit;        /* [n] */
  const int64_t* now;         /* [n] */
  const uint32_t* count;      /* [n] */
  const uint8_t* lc;          /* [n] */
} rl_restore_batch;

typedef struct rl_table_info {
  uint64_t table_slots;
  uint64_t live_slots;        /* occupied (non-empty, non-tombstone) slots */
  uint64_t tombstones;
  uint64_t arena_bytes_used;
  uint64_t exact_stems;       /* slots flagged multi-unit (exact slow path) */
  uint64_t batches;
  uint64_t decisions;
  uint64_t history_entries;   /* entries of the history log (rl_config.history_entries, rounded) */
  uint64_t history_appended;  /* records appended to the log since rl_create / rl_snapshot_load */
  uint64_t history_lost;      /* lookups that found an entry the log had overwritten: answered
                                 RL_E_TIME (size history_entries up) */
  uint64_t history_slots;     /* live slots with a history chain */
  uint64_t history_refused;   /* records the log refused: their partition had taken
                                 history_entries / 64 appends in one batch already (a batch's
                                 appends never wrap a partition onto its own entries); a later
                                 lookup of such a window is RL_E_TIME (size history_entries up) */
} rl_table_info;

typedef struct rl_ctx rl_ctx;

uint32_t rl_abi_version(void);

/* Create / destroy a backend on cfg->device. NULL on failure (message in err). */
rl_ctx* rl_create(const rl_config* cfg, char* err, size_t errlen);
void rl_destroy(rl_ctx* ctx);
const char* rl_last_error(const rl_ctx* ctx);

/* DoLimit for a whole batch. Host buffers (pinned via rl_alloc_host is fastest).
 * Synchronous: returns after results are in *out.
 * Multi-GPU (rl_config.n_shards > 1): the table is hash-sharded over
 * shard_device[0..n_shards) inside this one ctx (the reference's single service
 * process scaled out over a Redis cluster, src/redis/driver_impl.go:108-126).
 * Each shard has a worker thread and a router; the shards' routers form an
 * in-process world (the loopback transport: device copies, over xGMI between
 * distinct devices). A host batch is cut into one request-aligned slice per
 * shard; each shard copies its slice over its own device's link, partitions
 * it by owner, exchanges records with the other shards, runs the pipeline on
 * the keys it owns, and returns the answers to the slice's source, which
 * writes them to *out in arrival order; the stats of the slices are summed.
 * Same call, same answers. Owners keep stats per source slice, so every shard
 * is created with n_shards x max_rules rows (a batch may carry max_rules). */
int rl_do_limit(rl_ctx* ctx, const rl_batch* in, rl_result* out);

/* Same, with every pointer in *in / *out in device memory of ctx's GPU
 * (shard_device[0] when n_shards > 1), pipelined on the ctx's own streams.
 * With `stream` (a hipStream_t) the batch starts after the work already on it
 * (the inputs' producer); with NULL the inputs must be complete at the call.
 * *out is read after rl_synchronize (the caller's stream is never made to wait
 * for a batch, which would chain the next batch's inputs behind it and
 * serialise the pipeline). The inputs are read until the batch is complete
 * (rl_synchronize, or rl_batch_progress): keep them unchanged until then.
 * Returns once the work is enqueued; errors detected
 * on the GPU surface at rl_synchronize. On a multi-shard ctx shard 0 takes the
 * whole device batch as its slice (the other shards' slices are empty) and
 * routes it to the owners as above; the caller's thread waits only until every
 * shard's worker has enqueued its part, never for the GPU.
 * stem_bytes must be 4-byte aligned (any hipMalloc / torch allocation is). */
int rl_do_limit_async(rl_ctx* ctx, const rl_batch* in, rl_result* out, void* stream);

/* Host buffers in and out, like rl_do_limit, without waiting: the batch's
 * inputs cross PCIe into one of the ctx's device staging slots while earlier
 * batches compute, its outputs cross back when it is done; *out is read after
 * rl_synchronize, and the host buffers of a batch stay untouched until then.
 * Pinned buffers (rl_alloc_host) make the copies asynchronous. The fed path of
 * a batcher whose requests arrive in host memory. On a multi-shard ctx each
 * shard's worker copies its request-aligned slice over its own link and routes
 * it (rl_do_limit); out->stats is written at rl_synchronize (or once the
 * ring of batches in flight comes round to this batch again).
 * On a multi-shard ctx rl_synchronize, rl_sweep, rl_restore, the info getters
 * and the snapshot calls first complete every shard's pending batches. */
int rl_do_limit_host_async(rl_ctx* ctx, const rl_batch* in, rl_result* out);
int rl_synchronize(rl_ctx* ctx);

/* Pipelined batchers (single-shard ctx): the number of batches submitted
 * through rl_do_limit* so far and how many of them, in submission order, have
 * their outputs complete (host-fed batches: copied back). Never waits, so a
 * batcher can hand out the answers of finished batches while later ones run;
 * device-side errors are still reported by rl_synchronize. */
int rl_batch_progress(rl_ctx* ctx, uint64_t* submitted, uint64_t* completed);

/* ---- Compact host batch: the fed path's PCIe format ---------------------
 * The same batch as rl_batch, laid out for the link: ONE contiguous host
 * buffer (one copy per batch), per request its clock, HitsAddend and first
 * descriptor (the reference's per-request fields, RateLimitRequest.HitsAddend
 * and the UnixNow() of the DoLimit call, fixed_cache_impl.go:33-51), per
 * descriptor its stem and a 16-bit index into a table of the batch's distinct
 * limits (a config rule, or an interned per-request override): 46 B per
 * descriptor at BASELINE C1 (34-B stems, two descriptors per request) against
 * rl_batch's 60. Answers, errors and statuses are those of the equivalent
 * rl_batch (a limit index >= n_limits is an RL_E_INVALID descriptor). */
typedef struct rl_limit {
  uint32_t requests_per_unit;  /* RateLimit.Limit.RequestsPerUnit */
  uint32_t rule_id;            /* stats row of the limit (< n_rules) */
  uint8_t unit;                /* rl_unit */
  uint8_t flags;               /* RL_FLAG_* */
  uint16_t reserved;
} rl_limit;

/* Sections of buf, as byte offsets (each a multiple of 4, in any order). */
typedef struct rl_batch_compact {
  uint32_t n;            /* descriptors */
  uint32_t n_requests;
  uint32_t n_rules;
  uint32_t n_limits;     /* entries of the limit table (<= 65536) */
  const uint8_t* buf;    /* pinned host memory (rl_alloc_host): copied once, asynchronously */
  uint64_t buf_bytes;
  uint64_t stem_bytes;   /* concatenated stems */
  uint64_t stem_off;     /* uint32[n + 1], stem_off[0] == 0 */
  uint64_t limit_idx;    /* uint16[n] */
  uint64_t req_first;    /* uint32[n_requests + 1]: request q holds descriptors
                            [req_first[q], req_first[q+1]); req_first[0] == 0,
                            non-decreasing, req_first[n_requests] == n */
  uint64_t now;          /* uint32[n_requests] UnixNow() (< 2^32 - 172800, as rl_batch.now) */
  uint64_t hits;         /* uint32[n_requests] HitsAddend */
  uint64_t limits;       /* rl_limit[n_limits] */
} rl_batch_compact;

/* rl_do_limit_host_async on a compact batch: on a single-shard ctx buf
 * crosses PCIe in one copy into a device staging slot while earlier batches
 * compute, is unpacked on the GPU, and the batch is pipelined like any other.
 * On a multi-shard ctx it is cut into one request-aligned slice per shard;
 * each shard copies its slice's parts of buf over its own device's link,
 * unpacks them and routes them like an rl_batch host slice. *out is read
 * after rl_synchronize; buf stays untouched until then. Not on a ctx that
 * joined a communicator (rl_do_limit_routed_async takes device batches). */
int rl_do_limit_compact_async(rl_ctx* ctx, const rl_batch_compact* in, rl_result* out);

/* ---- Prefix-shared batch: the densest PCIe format ----------------------
 * Every descriptor of one RateLimitRequest starts with the same
 * prefix ‖ domain ‖ '_' and, in practice, with its request's leading entries
 * (cache_key.go:62-71; nested descriptors repeat their parents'). This layout
 * stores those shared bytes once per request and each descriptor's remaining
 * suffix: descriptor d of request q has the stem prefix[q] ‖ suffix[d]. Per
 * request: descriptor count and prefix length (one u32), UnixNow(), HitsAddend;
 * per descriptor: one u32 (limit index, suffix length). 31.5 B per decision at
 * BASELINE C1 (25-B shared prefix, two 9-B suffixes) against rl_batch_compact's
 * 46 and rl_batch's 60. Requests form tiles of RL_PREFIXED_TILE; the index
 * holds each tile's starting offsets, which the batcher has at hand while it
 * appends, so the GPU unpacks every tile independently (no scan pass) and a
 * multi-shard ctx cuts the batch at tile boundaries without reading it.
 * Answers, errors and statuses are those of the equivalent rl_batch (a limit
 * index >= n_limits, or a stem of 0 or more than 65535 bytes, is an
 * RL_E_INVALID descriptor; an index that does not match the sections fails
 * the batch with RL_E_INVALID at rl_synchronize). */
#define RL_PREFIXED_TILE 256u
typedef struct rl_batch_prefixed {
  uint32_t n;            /* descriptors */
  uint32_t n_requests;
  uint32_t n_rules;
  uint32_t n_limits;     /* entries of the limit table (<= 65536) */
  const uint8_t* buf;    /* pinned host memory (rl_alloc_host): copied once, asynchronously */
  uint64_t buf_bytes;
  /* sections of buf, as byte offsets (each a multiple of 4, in any order) */
  uint64_t req;          /* uint32[n_requests]: descriptors of the request (bits 0-15) | bytes of
                            its shared prefix (bits 16-23, at most 255) << 16; bits 24-31 zero.
                            A request's descriptors follow those of the request before it */
  uint64_t now;          /* uint32[n_requests] UnixNow() (< 2^32 - 172800, as rl_batch.now) */
  uint64_t hits;         /* uint32[n_requests] HitsAddend */
  uint64_t desc;         /* uint32[n]: limit index (bits 0-15) | suffix bytes (bits 16-31) << 16 */
  uint64_t prefix_bytes; /* the requests' shared prefixes, concatenated in request order */
  uint64_t suffix_bytes; /* the descriptors' suffixes, concatenated in descriptor order */
  uint64_t limits;       /* rl_limit[n_limits] */
  uint64_t index;        /* uint32[4 x (tiles + 1)], tiles = ceil(n_requests / RL_PREFIXED_TILE):
                            entry t = {first descriptor, first prefix byte, first suffix byte,
                            first byte of the unpacked stems} of requests [t x TILE, (t+1) x TILE);
                            entry 0 is zero, entry `tiles` the totals {n, prefix bytes, suffix
                            bytes, stem bytes (<= max_stem_bytes)} */
} rl_batch_prefixed;

/* rl_do_limit_compact_async's contract for a prefix-shared batch: buf crosses
 * PCIe in one copy (a multi-shard ctx: each shard copies the parts of its
 * tile-aligned slice over its own device's link), is unpacked on the GPU and
 * pipelined like any batch. *out is read after rl_synchronize; buf stays
 * untouched until then. Not on a ctx that joined a communicator. */
int rl_do_limit_prefixed_async(rl_ctx* ctx, const rl_batch_prefixed* in, rl_result* out);

/* Epoch sweep (replaces Redis EXPIRE): tombstones every slot whose counter
 * and local-cache entries have all expired at `now`; `now` becomes a floor
 * (later requests with an earlier time fail with RL_E_TIME). Inserts reuse
 * tombstones; when fewer than a quarter of the slots are empty after the
 * eviction, the sweep also turns every tombstone that no live key's probe path
 * crosses back into an empty slot (one more pass that rehashes the live stems),
 * so a table under key turnover keeps short probes and rl_table_info.tombstones
 * may fall from one sweep to the next. *n_evicted counts evicted keys only. */
int rl_sweep(rl_ctx* ctx, int64_t now, uint64_t* n_evicted);

/* Seed / restore counters (host buffers). */
int rl_restore(rl_ctx* ctx, const rl_restore_batch* in);

int rl_table_info_get(rl_ctx* ctx, rl_table_info* info);  /* summed over shards */
int rl_table_info_shard(rl_ctx* ctx, uint32_t shard, rl_table_info* info);

/* Pinned host memory for the packed buffers (hipHostMalloc). */
void* rl_alloc_host(size_t bytes);
void rl_free_host(void* p);

/* Diagnostics used by the parity tests (host buffers):
 * rl_debug_keys materialises each descriptor's full Redis key
 * (stem ‖ decimal window start) on the GPU into out_bytes/out_off (n+1). */
int rl_debug_keys(rl_ctx* ctx, const rl_batch* in, uint8_t* out_bytes, uint32_t* out_off,
                  uint32_t out_cap);
/* rl_debug_decide runs the device GetResponseDescriptorStatus on explicit
 * (before, after, local-cache flag) tuples: base_limiter.go:76-135. */
int rl_debug_decide(rl_ctx* ctx, uint32_t n, const uint32_t* before, const uint32_t* after,
                    const uint8_t* lc_hit, const uint32_t* hits, const uint32_t* limit,
                    const uint8_t* unit, const uint8_t* flags, const int64_t* now,
                    uint8_t* code, uint32_t* remaining, uint32_t* reset_s,
                    uint64_t* stat_deltas /* n * RL_NUM_STATS */, uint8_t* lc_set);
/* rl_debug_log_tear (tests; libraries built with RL_LOG_TEAR, else RL_E_INVALID):
 * replays a concurrent writer of a history-log entry between a lookup's loads.
 * With arm != NULL it arms a one-shot tear: the first entry the next lookup
 * (log_find) reads is overwritten by `entry`, the writer's steps applied by the
 * reading lane itself: sched[i] of them before the reader's i-th load (header,
 * record, header re-read; non-decreasing), the rest after its verdict. With
 * out != NULL (after the batches that should have fired it) it reads the
 * outcome back and disarms. The lookup uses a record only if the writer and
 * reader protocols keep header and record of one write together; the tests
 * check that over every schedule. */
typedef struct rl_log_tear {
  uint32_t armed;      /* in: 1; out: 2 once a lookup fired it */
  uint32_t protocol;   /* 0: the library's writer (header BUSY, record, header: 3 steps);
                          1: round 5's order (header, record: 2 steps) */
  uint32_t sched[3];   /* writer steps done before the reader's header load, record load, re-read */
  uint32_t entry[8];   /* the overwriting entry: slot, tag, prev, t_app, then the record ws, count,
                          expire, lc; 0xFFFFFFFF in slot / tag / prev / t_app = the entry's own */
  uint32_t before[8];  /* out: the entry before the tear */
  uint32_t seen[12];   /* out: the reader's header, record and header re-read */
  int32_t verdict;     /* out: 1 the record was used (its window), 0 the walk moved on, -1 rejected */
  uint32_t reserved;
} rl_log_tear;
int rl_debug_log_tear(rl_ctx* ctx, const rl_log_tear* arm, rl_log_tear* out);

/* ---- Multi-GPU routing across processes (one single-shard rl_ctx per GPU) ---
 * SURVEY.md §8e. For one process per GPU (torch.distributed / RCCL), each rank
 * routes its slice of the node's requests; the collectives are the caller's
 * (ratelimit_amd/sharded.py). Every pointer is device memory of ctx's GPU, work
 * is enqueued on `stream` (a hipStream_t, NULL = ctx's stream) and never waits
 * on the host; errors surface at rl_synchronize. Every rank's ctx must share
 * rl_config.hash_seed (owner = stem hash).
 *
 * rl_route_pack (source side): stable-partitions the batch `in` by owner shard
 * and writes, in owner order, one RL_WIRE_BYTES record per descriptor (its
 * fields, its request's clock as 32 bits, and the keyed 64-bit stem hash, so
 * owners never rehash; no stem offset) to send_rec and its stem bytes to
 * send_stem (capacity: the batch's stem bytes), each owner's stems in its
 * records' order.
 * perm[j] = batch index of record j. counts[2*d], [2*d+1] (device memory) =
 * records / stem bytes for owner d (all zero when the batch is malformed). Request
 * indices must be < 2^24; the global request label is src_rank << 24 | req_idx,
 * so chunks concatenated in source-rank order are in global arrival order.
 *
 * rl_route_do_limit (owner side): DoLimit over the n records received from all
 * sources (concatenated in source-rank order) with their stems (recv_stem,
 * 4-byte aligned, recv_stem_bytes long; src_stem_base = host array of each
 * source's chunk offset in recv_stem: the chunks abut in source order, and
 * each record's stem starts where the previous record's ends), pipelined on the ctx's streams once the
 * work already on `stream` is done; then, on `stream`, ret[j] = the packed
 * result of record j (bits 0-31 remaining, 32-51 reset_s, 52-55 status, 56-61
 * code, 62 local-cache hit). stats: rule_stride == 0: n_rules x RL_NUM_STATS
 * deltas; rule_stride > 0: per source rank, n_shards blocks of rule_stride x
 * RL_NUM_STATS (the deltas of each source's own requests). isolate != 0:
 * per-descriptor statuses (rl_result.status semantics) in ret.
 *
 * rl_route_scatter (source side): results returned in record order (ret, n =
 * the batch size) -> out (device SoA, status optional) in arrival order. */
#define RL_WIRE_BYTES 32u
#define RL_MAX_SHARDS 256u
int rl_route_pack(rl_ctx* ctx, const rl_batch* in, uint32_t n_shards, uint32_t src_rank, void* send_rec,
                  uint8_t* send_stem, uint32_t* perm, uint64_t* counts, void* stream);
int rl_route_do_limit(rl_ctx* ctx, uint32_t n, const void* recv_rec, const uint8_t* recv_stem,
                      uint64_t recv_stem_bytes, const uint64_t* src_stem_base, uint32_t n_shards, uint32_t n_rules,
                      uint32_t rule_stride, uint64_t* ret, uint64_t* stats, int isolate, void* stream);
int rl_route_scatter(rl_ctx* ctx, uint32_t n, const uint32_t* perm, const uint64_t* ret, rl_result* out,
                     void* stream);

/* ---- Multi-rank routing inside the library (RCCL or in-process loopback) ---
 * SURVEY.md §8e with the exchange itself in the library (rl_comm.hip): one
 * rank per table shard, each with one single-shard ctx, every ctx created with
 * the same rl_config.hash_seed.
 *
 * rl_comm_unique_id (one rank) fills RL_COMM_ID_BYTES bytes (an ncclUniqueId)
 * that the caller hands to every rank (e.g. a torch.distributed broadcast):
 * one process per GPU, exchanges over RCCL (xGMI). RCCL is loaded then
 * (dlopen), not at library load.
 * rl_comm_loopback_id fills the id of an in-process world instead: its ranks
 * are threads of THIS process, one ctx each (any devices; several may share
 * one GPU, which RCCL refuses), exchanging by device copies with the same
 * protocol. A rank whose peers never arrive fails with RL_E_COMM after
 * RL_LOOPBACK_TIMEOUT_S seconds (default 120) instead of waiting forever.
 * rl_comm_init (collective: every rank, the same id) joins ctx to the world as
 * `rank`.
 *
 * rl_do_limit_routed_async (collective: every rank calls it the same number of
 * times in the same order; n may be 0) answers this rank's slice of the node
 * batch. Rank r's slice precedes rank r+1's in the global order (the order the
 * sequential INCRBY contract is kept in). Device arrays; the batch starts
 * after the work already on `stream` (NULL: inputs complete at the call). A
 * call enqueues its batch's partition and counts exchange and completes the
 * batch RL_ROUTED_LAG calls back, so the host never waits for work it just
 * issued and that many owner pipelines stay queued on the GPU. The
 * descriptors a rank owns of its own slice are read in place by its owner
 * batch (no copy): a batch's inputs may be reused once RL_ROUTED_INFLIGHT
 * later calls have returned, or after rl_synchronize; its outputs are read
 * after rl_synchronize (collective too on such a ctx: it completes the last
 * batch). Keep `out` valid until then. out->stats = the deltas of
 * THIS rank's requests (summed over ranks: the node's). Ranks may pass
 * different n_rules; every owner keeps stats per source with the largest
 * n_rules of the batch as stride, so it needs max_rules >= world x that. If
 * any rank passes out->status, owners answer per descriptor (isolation) for
 * the whole batch.
 * Errors never leave a peer waiting: a slice this rank rejects (sizes, null
 * outputs) takes part in the exchange with no records and fails this rank's
 * batch at rl_synchronize; an owner that cannot run what it received answers
 * every such record with its rl_status (in out->status, or failing the
 * source's batch at rl_synchronize). Only a HIP / transport runtime failure
 * leaves the ctx's router unusable (RL_E_COMM / RL_E_HIP from every later
 * call). Replaces the Redis cluster client's key-slot routing inside one
 * service process (src/redis/driver_impl.go:108-126).
 * On a routed ctx rl_synchronize, rl_sweep, rl_restore and rl_snapshot_save /
 * _load first complete the pending batches, so they are collective like the
 * batches. rl_sweep there applies one floor on every rank: the least `now`
 * the ranks passed (a rank passing an out-of-range time fails alone and does
 * not vote), so a rank's requests are never refused by an owner whose clock
 * runs ahead of its own. The read-only getters rl_table_info_get and rl_local_cache_info_get
 * are not: they see every batch but the pending ones (the last RL_ROUTED_LAG
 * submitted), and a rank may call them alone (e.g. for its gauges). */
#define RL_COMM_ID_BYTES 128u
#ifndef RL_ROUTED_INFLIGHT       /* (overridable only for A/B builds of the library) */
#define RL_ROUTED_INFLIGHT 6u  /* routed batches in flight (the input-reuse distance above) */
#endif
#ifndef RL_ROUTED_LAG
#define RL_ROUTED_LAG 3u       /* calls between a routed batch's partition and its owner pipeline */
#endif
int rl_comm_unique_id(uint8_t* id);
int rl_comm_loopback_id(uint8_t* id);
int rl_comm_init(rl_ctx* ctx, uint32_t world, uint32_t rank, const uint8_t* id);
int rl_do_limit_routed_async(rl_ctx* ctx, const rl_batch* in, rl_result* out, void* stream);

/* ---- Config match on the GPU (the caller side of DoLimit) ---
 * The service's constructLimitsToCheck (src/service/ratelimit.go:104-143) calls
 * rateLimitConfigImpl.GetLimit (src/config/config_impl.go:243-298) once per
 * descriptor, then DoLimit, then maps unlimited descriptors to
 * {OK, LimitRemaining = MaxUint32} (ratelimit.go:176-183). rl_do_limit_requests
 * does all three on the device for a batch of raw requests: the host only
 * copies domain / entry bytes; the config trie is walked per descriptor on the
 * GPU and the matched descriptors are compacted into the DoLimit pipeline.
 *
 * rl_config_load replaces the loaded config (GetCurrentConfig snapshot,
 * ratelimit.go:105) with a flattened trie: one rl_config_node per domain root
 * and per descriptor config node (rateLimitDescriptor, config_impl.go:45-48),
 * parents before children. A node's key is the domain name for a root, else
 * its finalKey: key, or key ‖ '_' ‖ value (config_impl.go:106-109). Host
 * buffers; (parent, key) pairs must be unique (RL_E_INVALID otherwise).
 * cache_key_prefix is CACHE_KEY_PREFIX (cache_key.go:62, settings.go). */
typedef struct rl_config_node {
  int32_t parent;             /* index of the parent node; -1: a domain root */
  uint32_t key_off;           /* key bytes in rl_config_tree.key_bytes */
  uint32_t key_len;
  uint32_t requests_per_unit; /* RateLimit.Limit.RequestsPerUnit */
  uint32_t rule_id;           /* dense id of the rule's Stats.Key (its full key path, config_impl.go:111,139) */
  uint8_t unit;               /* rl_unit (0 for unlimited) */
  uint8_t has_limit;          /* the node has a rate_limit block (rateLimitDescriptor.limit != nil) */
  uint8_t unlimited;          /* RateLimit.Unlimited */
  uint8_t shadow_mode;        /* RateLimit.ShadowMode */
} rl_config_node;

typedef struct rl_config_tree {
  uint32_t n_nodes;
  uint32_t cache_key_prefix_len;
  const rl_config_node* nodes;
  const uint8_t* key_bytes;
  uint64_t key_bytes_len;
  const uint8_t* cache_key_prefix;
} rl_config_tree;

int rl_config_load(rl_ctx* ctx, const rl_config_tree* tree);

/* Raw requests (RateLimitRequest, arrival order). Descriptor d belongs to
 * request req_idx[d] (non-decreasing); its entries are
 * [entry_first[d], entry_first[d+1]), and its bytes
 * desc_bytes[desc_off[d], desc_off[d+1]) (all offsets non-decreasing) are Σ(key ‖ '_' ‖ value ‖ '_') over its
 * entries (the stem tail of cache_key.go:65-70), with key_len / value_len per
 * entry. Overrides (RateLimitDescriptor.Limit, config_impl.go:255-266):
 * override_flags[d] bit 0 = present, with override_rpu / override_unit and
 * override_rule = dense id of descriptorKey(domain, descriptor) (interned
 * host-side: the one per-override string the caller builds). The three
 * override arrays may be NULL when no descriptor carries one. Host buffers. */
typedef struct rl_request_batch {
  uint32_t n_requests;
  uint32_t n_descriptors;
  uint32_t n_entries;
  uint32_t n_rules;               /* every rule id (config and override) < n_rules */
  const uint8_t* domain_bytes;    /* RateLimitRequest.Domain, concatenated */
  const uint32_t* domain_off;     /* [n_requests + 1] */
  const int64_t* now;             /* [n_requests] UnixNow() of each request */
  const uint32_t* hits;           /* [n_requests] HitsAddend */
  const uint32_t* req_idx;        /* [n_descriptors] */
  const uint32_t* entry_first;    /* [n_descriptors + 1] */
  const uint32_t* desc_off;       /* [n_descriptors + 1] */
  const uint8_t* desc_bytes;
  const uint16_t* key_len;        /* [n_entries] */
  const uint16_t* value_len;      /* [n_entries] */
  const uint8_t* override_flags;  /* [n_descriptors] or NULL */
  const uint32_t* override_rpu;   /* [n_descriptors] or NULL */
  const uint8_t* override_unit;   /* [n_descriptors] or NULL (pb_type.RateLimitUnit) */
  const uint32_t* override_rule;  /* [n_descriptors] or NULL */
} rl_request_batch;

/* Per descriptor, what the service answers (ratelimit.go:158-190). */
enum rl_match { RL_MATCH_NONE = 0, RL_MATCH_UNLIMITED = 1, RL_MATCH_LIMIT = 2 };
typedef struct rl_request_result {
  uint8_t* code;               /* [n_descriptors] rl_code */
  uint32_t* limit_remaining;   /* [n_descriptors]; MaxUint32 for unlimited */
  uint32_t* reset_s;           /* [n_descriptors]; 0 = no DurationUntilReset (nil limit) */
  uint8_t* match;              /* [n_descriptors] rl_match */
  uint32_t* rule_id;           /* [n_descriptors] matched rule (RL_MATCH_LIMIT / UNLIMITED) */
  uint32_t* requests_per_unit; /* [n_descriptors] CurrentLimit.RequestsPerUnit (RL_MATCH_LIMIT) */
  uint8_t* unit;               /* [n_descriptors] CurrentLimit.Unit (RL_MATCH_LIMIT) */
  uint64_t* stats;             /* [n_rules * RL_NUM_STATS], this call's deltas */
} rl_request_result;

/* GetLimit + DoLimit + the unlimited mapping for a batch of raw requests.
 * Synchronous. A descriptor whose override or config unit is not 1..4 fails
 * the batch with RL_E_INVALID (the reference panics in UnitToDivider). On a
 * multi-shard ctx the match runs on shard 0's GPU and the matched descriptors
 * go through the shards like a device batch (every owner answers its keys);
 * not on a ctx that joined a communicator. */
int rl_do_limit_requests(rl_ctx* ctx, const rl_request_batch* in, rl_request_result* out);

/* The rest of shouldRateLimitWorker per request (ratelimit.go:163-209, with
 * customHeadersEnabled): RateLimitResponse.OverallCode, the descriptor
 * "closest to its limit" whose values the RateLimit-Limit / -Remaining / -Reset
 * headers carry (minimumDescriptor, :165-176 and :185-190; the header values,
 * :194-201 and :213-237), and global SHADOW_MODE with its global_shadow_mode
 * counter (:203-207). Request q's descriptors are the d with req_idx[d] == q
 * (contiguous, in order):
 *  - some d has match == RL_MATCH_LIMIT and code == RL_CODE_OVER_LIMIT:
 *    finalCode OVER_LIMIT, minimumDescriptor = the last such d;
 *  - otherwise finalCode OK and minimumDescriptor = the first d with match ==
 *    RL_MATCH_LIMIT and the smallest limit_remaining (the reference compares
 *    with a strict <, starting from MaxUint32: a remaining of MaxUint32 is
 *    never chosen); none: RL_NO_DESCRIPTOR and header values 0. Unlimited and
 *    unmatched descriptors have no CurrentLimit and are never chosen.
 * header_reset_s is that descriptor's own reset_s: the reference reads its
 * header clock a moment after DoLimit's, this backend has one clock per request.
 * With RL_VERDICT_OPT_GLOBAL_SHADOW an OVER_LIMIT finalCode is answered OK,
 * flagged RL_VERDICT_OVER_LIMIT | RL_VERDICT_GLOBAL_SHADOW and counted in
 * *global_shadow; the headers stay as computed. A request without descriptors:
 * OK, RL_NO_DESCRIPTOR, flags 0. */
#define RL_NO_DESCRIPTOR 0xFFFFFFFFu
#define RL_VERDICT_OVER_LIMIT    0x1u  /* finalCode was OVER_LIMIT before global shadow mode */
#define RL_VERDICT_GLOBAL_SHADOW 0x2u  /* ... and global shadow mode turned it into OK */
#define RL_VERDICT_OPT_GLOBAL_SHADOW 0x1u  /* opts: settings SHADOW_MODE (ratelimit.go:203) */

typedef struct rl_request_verdict {   /* host memory, one entry per request */
  uint8_t*  overall_code;      /* [n_requests] rl_code: RateLimitResponse.OverallCode */
  uint8_t*  flags;             /* [n_requests] RL_VERDICT_* (may be NULL) */
  uint32_t* min_descriptor;    /* [n_requests] batch index of minimumDescriptor, RL_NO_DESCRIPTOR if nil (may be NULL) */
  uint32_t* header_limit;      /* [n_requests] its CurrentLimit.RequestsPerUnit (may be NULL) */
  uint32_t* header_remaining;  /* [n_requests] its LimitRemaining (may be NULL) */
  uint32_t* header_reset_s;    /* [n_requests] its DurationUntilReset seconds (may be NULL) */
  uint64_t* global_shadow;     /* [1] requests flagged RL_VERDICT_GLOBAL_SHADOW: stats.GlobalShadowMode.Add (may be NULL) */
} rl_request_verdict;

/* rl_do_limit_requests plus the verdict (same table effects, stats and
 * per-descriptor answers; synchronous; multi-shard: the verdict runs on shard
 * 0 after the expansion; not on a ctx that joined a communicator). out may be
 * NULL, as may any array in it: those are not copied back, so that with
 * out == NULL only per-request bytes return to the host. verdict and
 * verdict->overall_code are required (RL_E_INVALID). A batch that fails writes
 * nothing to *verdict's arrays. */
int rl_do_limit_requests_verdict(rl_ctx* ctx, const rl_request_batch* in, rl_request_result* out,
                                 uint32_t opts, rl_request_verdict* verdict);
/* ---- One-buffer raw requests: the request path, pipelined ---------------
 * The batch of rl_request_batch laid out for the link, like rl_batch_prefixed:
 * one pinned buffer that crosses PCIe in one copy and is unpacked on the GPU.
 * req_idx, entry_first, desc_off and domain_off do not cross: a request
 * carries its descriptor count and domain length, a descriptor its entry
 * count, and a descriptor's bytes are the sum of key_len + value_len + 2 over
 * its entries. key_len, value_len, the domain bytes and the entry bytes are
 * used where they land on the device. Requests form tiles of RL_REQUESTS_TILE;
 * the index holds each tile's starting offsets, so every tile is unpacked
 * independently. Overrides (RateLimitDescriptor.Limit) are a sparse list.
 * Answers, errors and statuses are those of rl_do_limit_requests_verdict on
 * the equivalent rl_request_batch. Malformed input:
 *  - a section outside buf or not 4-byte aligned, an index whose entry 0 is
 *    not zero or whose last entry is not {n_descriptors, n_entries, domain
 *    bytes, entry bytes}: RL_E_INVALID at the call;
 *  - sizes over max_batch / max_requests / max_rules, entry bytes over
 *    max_stem_bytes: RL_E_CAPACITY at the call;
 *  - a tile whose index entry does not match the sums of its requests'
 *    descriptor counts and domain lengths, its descriptors' entry counts or
 *    its entries' lengths; an override whose descriptor is >= n_descriptors or
 *    not above the one before it, or whose reserved bytes are not zero: the
 *    batch fails with RL_E_INVALID at rl_synchronize, the table untouched. */
#define RL_REQUESTS_TILE 256u
typedef struct rl_request_override {   /* sparse: only descriptors carrying RateLimitDescriptor.Limit */
  uint32_t descriptor;                 /* batch index, strictly increasing over the list */
  uint32_t requests_per_unit;
  uint32_t rule_id;                    /* override_rule of rl_request_batch */
  uint8_t unit;                        /* pb_type.RateLimitUnit */
  uint8_t reserved[3];                 /* zero */
} rl_request_override;

typedef struct rl_request_batch_packed {
  uint32_t n_requests;
  uint32_t n_descriptors;
  uint32_t n_entries;
  uint32_t n_rules;         /* every rule id (config and override) < n_rules */
  uint32_t n_overrides;
  uint32_t reserved;        /* zero */
  const uint8_t* buf;       /* pinned host memory (rl_alloc_host): copied once, asynchronously */
  uint64_t buf_bytes;
  /* sections of buf, as byte offsets (each a multiple of 4, in any order) */
  uint64_t req;             /* uint32[n_requests]: descriptors of the request (bits 0-15) | bytes of
                               its domain (bits 16-31) << 16. A request's descriptors follow those
                               of the request before it */
  uint64_t now;             /* uint32[n_requests] UnixNow() (< 2^32 - 172800, as rl_batch.now) */
  uint64_t hits;            /* uint32[n_requests] HitsAddend */
  uint64_t desc;            /* uint16[n_descriptors]: entries of the descriptor; a descriptor's
                               entries follow those of the descriptor before it */
  uint64_t key_len;         /* uint16[n_entries] */
  uint64_t value_len;       /* uint16[n_entries] */
  uint64_t domain_bytes;    /* the requests' domains, concatenated in request order */
  uint64_t entry_bytes;     /* Σ(key ‖ '_' ‖ value ‖ '_') in entry order: rl_request_batch.desc_bytes */
  uint64_t overrides;       /* rl_request_override[n_overrides] */
  uint64_t index;           /* uint32[4 x (tiles + 1)], tiles = ceil(n_requests / RL_REQUESTS_TILE):
                               entry t = {first descriptor, first entry, first domain byte, first
                               entry byte} of requests [t x TILE, (t+1) x TILE); entry 0 is zero,
                               entry `tiles` the totals {n_descriptors, n_entries, domain bytes,
                               entry bytes (<= max_stem_bytes)} */
} rl_request_batch_packed;

/* rl_request_batch -> rl_request_batch_packed: writes the sections and the
 * tile index into buf and fills *out (out->buf = buf). Host code; no GPU
 * needed. A batcher runs rl_packer_pack and then this; `in` is only read.
 * buf == NULL or buf_cap too small: RL_E_CAPACITY with out->buf_bytes = the
 * bytes needed and nothing else written. RL_E_INVALID (nothing written):
 * offsets that do not start at 0, are not monotone or do not end at
 * n_entries; req_idx decreasing or >= n_requests; a request with more than
 * 65535 descriptors, a descriptor with more than 65535 entries, a domain
 * longer than 65535 bytes; a descriptor whose desc_off span is not the sum of
 * its entries' lengths plus separators; a now outside [0, 2^32). Only bit 0
 * of override_flags travels. */
int rl_request_batch_pack(const rl_request_batch* in, uint8_t* buf, uint64_t buf_cap,
                          rl_request_batch_packed* out);

/* rl_do_limit_requests_verdict on a packed batch, without waiting: the call
 * returns once the batch's copy, unpack and config match are enqueued. The
 * DoLimit pipeline needs the matched count on the host, so a batch's second
 * half (pipeline, expansion, verdict, outputs) is enqueued by a later call of
 * this entry point, by rl_batch_progress or by rl_synchronize, in submission
 * order, once its count has arrived; at most RL_REQUESTS_INFLIGHT batches wait
 * for theirs (a further call waits for the oldest one's count only). Every
 * other entry point first completes the pending batches, so calls interleaved
 * with other paths keep submission order. out and verdict may each be NULL
 * (not both), as may any array inside them: those are not copied back. *out
 * and *verdict are read after rl_synchronize, or once rl_batch_progress counts
 * the batch complete; buf stays untouched until then, and so must *in's index
 * until the call returns. A batch that fails in the match stage (malformed
 * content, matched stems over max_stem_bytes) skips its second half and leaves
 * the table untouched; the next rl_synchronize reports the first such failure
 * since the last one, that batch's outputs are unspecified and later batches
 * run normally. Pipeline-stage failures are those of rl_do_limit_host_async.
 * Single-shard ctxs only: a multi-shard ctx or one that joined a communicator
 * gets RL_E_INVALID (use rl_do_limit_requests_verdict there). */
#ifndef RL_REQUESTS_INFLIGHT
#define RL_REQUESTS_INFLIGHT 4u
#endif
int rl_do_limit_requests_packed_async(rl_ctx* ctx, const rl_request_batch_packed* in,
                                      rl_request_result* out, uint32_t opts,
                                      rl_request_verdict* verdict);

/* ---- Serialized requests parsed on the GPU ---------------------------------
 * The request path from the gRPC payloads themselves: the serialized
 * envoy.service.ratelimit.v3.RateLimitRequest messages cross PCIe as they
 * arrived, in one pinned buffer with one offset and one clock per request, and
 * are parsed on the device into what rl_packer_pack and rl_request_batch_pack
 * build on the host. The host reads the two ends of msg_off and no payload byte.
 *
 * Per-message status (wire->req_status), defined by the host packer:
 *  - RL_WIRE_MALFORMED exactly where rl_packer_pack on that message alone
 *    returns RL_E_INVALID;
 *  - RL_WIRE_DEFERRED for a well-formed message that carries a descriptor with
 *    `limit` (its stats key is a host-interned string; see
 *    rl_override_rules_enable for interning it on the device) or exceeds the packed
 *    layout's per-item limits (more than 65535 descriptors, a descriptor of
 *    more than 65535 entries, a domain over 65535 bytes): the caller resubmits
 *    it through the host packer;
 *  - RL_WIRE_OK otherwise, parsed as the packer parses it.
 * A deferred or malformed request takes part in the batch as a request
 * without descriptors: no table effect, no stats, desc_first[q + 1] ==
 * desc_first[q], the verdict entries of an empty request except
 * overall_code[q] = 0 (no rl_code), never counted in global_shadow. For
 * RL_WIRE_OK requests the answers, stats, statuses and table effects are
 * those of rl_do_limit_requests_packed_async on the batch rl_packer_pack and
 * rl_request_batch_pack make of the same messages with every other message
 * replaced by an empty one.
 *
 * Errors at the call (nothing enqueued): RL_E_INVALID for a null in, wire or
 * wire->req_status, out and verdict both null, a section outside buf or not
 * 4-byte aligned, msg_off[0] != 0 or msg_off[n_requests] != msgs_bytes, a
 * non-zero reserved field, unknown opts, no config loaded, a multi-shard ctx
 * or one that joined a communicator; RL_E_CAPACITY for n_requests >
 * max_requests or n_rules > max_rules. On the device: a decreasing msg_off
 * fails the batch with RL_E_INVALID at rl_synchronize; a batch of more
 * descriptors than min(desc_cap, max_batch) (desc_cap counts only with out
 * non-NULL) or more entry bytes than max_stem_bytes fails with RL_E_CAPACITY
 * there. A failed batch leaves the table untouched and later batches run
 * normally. out, verdict, rl_batch_progress, rl_synchronize and the order
 * against other entry points are those of rl_do_limit_requests_packed_async;
 * wire's arrays are read when out's and verdict's are. */
#define RL_WIRE_TILE 256u
enum rl_wire_status { RL_WIRE_OK = 0, RL_WIRE_DEFERRED = 1, RL_WIRE_MALFORMED = 2 };

typedef struct rl_wire_batch {
  uint32_t n_requests;
  uint32_t n_rules;      /* config rule ids are < n_rules; with rl_override_rules_enable, override rule ids too */
  const uint8_t* buf;    /* pinned host memory (rl_alloc_host): copied once, asynchronously */
  uint64_t buf_bytes;
  /* sections of buf, byte offsets, each a multiple of 4 */
  uint64_t msg_off;      /* uint32[n_requests + 1]: message q = msgs[msg_off[q], msg_off[q+1]); msg_off[0] == 0 */
  uint64_t now;          /* uint32[n_requests] UnixNow() (as rl_request_batch_packed.now) */
  uint64_t msgs;         /* the serialized RateLimitRequest payloads, concatenated */
  uint64_t msgs_bytes;   /* == msg_off[n_requests], < 2^32 */
} rl_wire_batch;

typedef struct rl_wire_result {   /* host memory */
  uint8_t*  req_status;    /* [n_requests] rl_wire_status; required */
  uint32_t* desc_first;    /* [n_requests + 1] first descriptor of each request in out's arrays; may be NULL */
  uint32_t* n_descriptors; /* [1] descriptors of the batch; may be NULL */
  uint32_t  desc_cap;      /* capacity, in descriptors, of out's per-descriptor arrays */
  uint32_t  reserved;      /* zero */
} rl_wire_result;

int rl_do_limit_wire_async(rl_ctx* ctx, const rl_wire_batch* in, rl_wire_result* wire,
                           rl_request_result* out, uint32_t opts, rl_request_verdict* verdict);

/* ---- Override stats keys interned on the GPU --------------------------------
 * A descriptor's `limit` override counts under the stats key
 * descriptorKey(domain, descriptor) (config_impl.go:300-312): domain '.' then,
 * per entry and joined by '.', key and, when the value is not empty, '_'
 * value. rl_packer_pack hands those keys dense rule ids on the host, which is
 * why the wire path defers such messages. rl_override_rules_enable moves that
 * interning onto the device: the ctx then owns a table of key bytes -> rule id
 * (ids first_rule, first_rule + 1, ... in the order the device first saw the
 * keys), and on both wire entry points a well-formed message whose descriptors
 * carry `limit` is RL_WIRE_OK when every one of its overrides
 *  - has a unit in 1..4 (another unit keeps the message RL_WIRE_DEFERRED: the
 *    host path keeps its behaviour for it),
 *  - has a descriptorKey of at most 65535 bytes,
 *  - found or was given a rule id r, and
 *  - r < in->n_rules,
 * and the message does not repeat a long domain over many overrides (each key
 * starts with the domain): overrides x (domain bytes + 1) <= 16 x the
 * message's bytes, which keeps a lane's work linear in its payload.
 * Otherwise the message is RL_WIRE_DEFERRED exactly as without the feature;
 * deferred_full counts the messages deferred by the last two conditions (no id
 * or arena space left, the bounded probe exhausted, r >= n_rules). No failure
 * of the interner fails a batch or yields a wrong id. For the RL_WIRE_OK
 * messages the answers, table effects, verdict, responses and stats are those
 * of rl_do_limit_requests_packed_async on the packer's batch of the same
 * messages, up to the naming of the override rule ids (compare rows by key).
 * requests_per_unit and unit merge across repeated `limit` fields as in the
 * packer; the domain is the message's last field 1.
 *
 * Identity is the key's bytes: entry ("a_b", "") and entry ("a", "b") give one
 * key and one id; two different keys never share an id (the full bytes are
 * compared; the hash, SipHash-1-3 under the ctx's hash_seed, only places
 * them). A key keeps its id for the ctx's lifetime. A malformed message
 * interns nothing; the keys of a batch that later fails at rl_synchronize stay
 * interned. Which new keys take the last free ids of a full table is
 * unspecified. An id is handed out even when it is >= the batch's n_rules
 * (that message is deferred; a later batch with a larger n_rules uses the id).
 *
 * The table is process state, like the reference's stats store: it is not part
 * of rl_snapshot_save / rl_snapshot_load, rl_export_range / rl_import or
 * rl_resize (which leaves it as it is), and rl_config_load does not move
 * first_rule: the caller reserves room for the config's rule ids below it.
 *
 * rl_override_rules_enable: once per ctx. RL_E_INVALID for a second call,
 * non-zero reserved fields, capacity == 0, first_rule + capacity > max_rules,
 * a multi-shard ctx or one that joined a communicator; RL_E_HIP when a device
 * allocation fails (nothing is enabled then). key_bytes above 2^32 - 1 is
 * taken as 2^32 - 1 (key_bytes_cap reports it). Without the call nothing
 * changes: a message with a `limit` is RL_WIRE_DEFERRED.
 *
 * rl_override_rules_info_get and rl_override_rule_keys order after every
 * submitted batch and are synchronous, like rl_lookup; RL_E_INVALID on a ctx
 * without the feature. rl_override_rule_keys returns the names of the ids
 * [from_rule, from_rule + n): key i = bytes[off[i], off[i+1]), off holding
 * n + 1 entries; RL_E_INVALID for a range outside [first_rule, first_rule +
 * rules); bytes == NULL or cap too small: RL_E_CAPACITY, *needed = the bytes
 * needed, off filled, no byte written (like rl_response_serialize). An adapter
 * fetches names only when an output shows a rule_id, or a non-zero stats row,
 * beyond the names it holds. */
typedef struct rl_override_rules_config {
  uint32_t first_rule;   /* ids handed out are first_rule, first_rule + 1, ... */
  uint32_t capacity;     /* at most this many distinct override stats keys */
  uint64_t key_bytes;    /* arena for their bytes (0 = 64 * capacity) */
  uint32_t reserved[4];  /* zero */
} rl_override_rules_config;
int rl_override_rules_enable(rl_ctx* ctx, const rl_override_rules_config* cfg);

typedef struct rl_override_rules_info {
  uint32_t first_rule, capacity, rules /* ids handed out */, reserved;
  uint64_t key_bytes_used, key_bytes_cap;
  uint64_t deferred_full;  /* messages deferred because no id / arena space / id >= n_rules */
} rl_override_rules_info;
int rl_override_rules_info_get(rl_ctx* ctx, rl_override_rules_info* info);

int rl_override_rule_keys(rl_ctx* ctx, uint32_t from_rule, uint32_t n, uint8_t* bytes, uint64_t cap,
                          uint32_t* off, uint64_t* needed /* may be NULL */);

/* ---- Serialized responses written on the GPU --------------------------------
 * The way back of the wire path: one serialized
 * envoy.service.ratelimit.v3.RateLimitResponse per request, as gRPC marshals
 * what shouldRateLimitWorker builds (ratelimit.go:161-210), written on the
 * device from the per-descriptor answers and the verdict. The bytes are the
 * canonical proto3 encoding (fields in field-number order, zero scalars and
 * empty strings omitted, minimal varints, a present sub-message written even
 * when empty). For a request q with RL_WIRE_OK:
 *   08 c                                  overall_code[q]
 *   per descriptor, in order:  12 L body  body = 08 code
 *                                           [12 M [08 requests_per_unit] 10 unit]   match == RL_MATCH_LIMIT
 *                                           [18 limit_remaining]                    non-zero
 *                                           [22 N [08 reset_s]]                     match == RL_MATCH_LIMIT
 *   with header keys and min_descriptor[q] != RL_NO_DESCRIPTOR, three
 *   HeaderValues (limit, remaining, reset):  1a H [0a klen key] 12 vlen digits
 *   the digits being the decimal ASCII of header_limit / _remaining / _reset_s.
 * A status has at most RL_RESPONSE_STATUS_MAX bytes (durations are below 2^21
 * seconds: the longest window is a day). A deferred or malformed request gets
 * an empty response (the host answers it itself); an RL_WIRE_OK request
 * without descriptors answers 08 01. */
#define RL_RESPONSE_KEY_MAX 64u
#define RL_RESPONSE_STATUS_MAX 26u

typedef struct rl_response_format {   /* read and copied at the call */
  const uint8_t* limit_key;      /* the three header names; all NULL (or a NULL format): no headers */
  const uint8_t* remaining_key;
  const uint8_t* reset_key;
  uint16_t limit_key_len;        /* each <= RL_RESPONSE_KEY_MAX; a NULL key's length is zero */
  uint16_t remaining_key_len;
  uint16_t reset_key_len;
  uint16_t reserved;             /* zero */
} rl_response_format;

typedef struct rl_response_batch {    /* host memory */
  uint8_t*  bytes;       /* pinned (rl_alloc_host): response q = bytes[resp_off[q], resp_off[q+1]) */
  uint64_t  bytes_cap;   /* >= rl_response_bound(n_requests, the batch's descriptors, fmt) */
  uint32_t* resp_off;    /* [n_requests + 1]; resp_off[0] == 0 */
} rl_response_batch;

/* No batch of n_requests requests over n_descriptors descriptors serializes to
 * more: n_requests x (2 + 3 x 16 + the key lengths) + 26 x n_descriptors with
 * headers, 2 x n_requests + 26 x n_descriptors without. Host code. */
uint64_t rl_response_bound(uint32_t n_requests, uint32_t n_descriptors, const rl_response_format* fmt);

/* rl_do_limit_wire_async plus the responses. out and verdict may both be NULL
 * here (the device computes the verdict either way); wire is required as
 * there. Only the used bytes of resp->bytes and resp_off cross PCIe; both are
 * read when out's and verdict's arrays are. Errors at the call (nothing
 * enqueued): those of rl_do_limit_wire_async, and RL_E_INVALID for a null
 * resp, resp->bytes or resp->resp_off, bytes not page-locked over bytes_cap,
 * a key over RL_RESPONSE_KEY_MAX bytes, a NULL key with a length, or a
 * non-zero reserved field. The response length depends on the counters, so
 * the capacity is checked by the bound once the descriptor count is known: a
 * batch whose rl_response_bound exceeds bytes_cap or does not fit 32 bits
 * fails with RL_E_CAPACITY at rl_synchronize, the table untouched, and later
 * batches run normally. Single-shard ctxs only. */
int rl_do_limit_wire_respond_async(rl_ctx* ctx, const rl_wire_batch* in, rl_wire_result* wire,
                                   rl_request_result* out, uint32_t opts, rl_request_verdict* verdict,
                                   const rl_response_format* fmt, rl_response_batch* resp);

/* The host twin: the same bytes and offsets from answers in host arrays
 * (request q's descriptors are [desc_first[q], desc_first[q+1]) of res's
 * arrays). It serves the deferred requests that go through the host packer,
 * and callers of the array paths. req_status may be NULL (every request
 * RL_WIRE_OK). res needs code, limit_remaining, reset_s, match,
 * requests_per_unit and unit; verdict needs overall_code and, with header
 * keys, min_descriptor and the three header arrays (RL_E_INVALID). bytes ==
 * NULL or bytes_cap too small: RL_E_CAPACITY, *bytes_needed = the exact bytes
 * needed, resp_off filled, no byte written. Host code; no GPU needed. */
int rl_response_serialize(uint32_t n_requests, const uint32_t* desc_first, const uint8_t* req_status,
                          const rl_request_result* res, const rl_request_verdict* verdict,
                          const rl_response_format* fmt, uint8_t* bytes, uint64_t bytes_cap,
                          uint32_t* resp_off, uint64_t* bytes_needed);

/* Diagnostics, like rl_debug_verdict: the device verdict and the device
 * serializer on explicit per-descriptor answers in host arrays (answers: code,
 * limit_remaining, reset_s, match, requests_per_unit, unit; reset_s < 2^21).
 * req_status may be NULL. Synchronous; resp->bytes may be pageable here.
 * RL_E_CAPACITY if rl_response_bound exceeds resp->bytes_cap. */
int rl_debug_respond(rl_ctx* ctx, uint32_t n_requests, uint32_t n_descriptors, const uint32_t* req_idx,
                     const uint8_t* req_status, const rl_request_result* answers, uint32_t opts,
                     const rl_response_format* fmt, rl_response_batch* resp);

/* Diagnostics (parity tests, like rl_debug_decide): the device verdict alone on
 * explicit per-descriptor answers in host arrays. req_idx must be non-decreasing
 * and < n_requests (RL_E_INVALID); n_descriptors <= max_batch and n_requests <=
 * max_requests (RL_E_CAPACITY). */
int rl_debug_verdict(rl_ctx* ctx, uint32_t n_requests, uint32_t n_descriptors, const uint32_t* req_idx,
                     const uint8_t* match, const uint8_t* code, const uint32_t* limit_remaining,
                     const uint32_t* reset_s, const uint32_t* requests_per_unit, uint32_t opts,
                     rl_request_verdict* verdict);

/* ---- Host packer -------------------------------------
 * Serialized envoy.service.ratelimit.v3.RateLimitRequest messages (the gRPC
 * payloads: msgs[msg_off[i], msg_off[i+1]), n + 1 offsets) with each request's
 * UnixNow() -> an rl_request_batch for rl_do_limit_requests, without building
 * per-descriptor objects. Replaces the per-descriptor Go work of
 * constructLimitsToCheck's caller side (src/service/ratelimit.go:104-143) and the
 * proto unmarshalling of the request. Override stats keys (descriptorKey,
 * src/config/config_impl.go:300-312) are interned to rule ids from
 * first_override_rule up (config rules take the ids below it);
 * rl_packer_rule_key names them. The batch's arrays are owned by the packer and
 * valid until its next rl_packer_pack. Host code; no GPU needed. */
typedef struct rl_packer rl_packer;
rl_packer* rl_packer_create(uint32_t first_override_rule);
void rl_packer_destroy(rl_packer* packer);
int rl_packer_pack(rl_packer* packer, const uint8_t* msgs, const uint64_t* msg_off, uint32_t n,
                   const int64_t* now, rl_request_batch* out);
uint32_t rl_packer_rules(const rl_packer* packer);  /* first_override_rule + interned override keys */
const char* rl_packer_rule_key(const rl_packer* packer, uint32_t rule_id);  /* NULL below first_override_rule */
const char* rl_packer_last_error(const rl_packer* packer);

/* ---- Observability and restart -----------------------
 * rl_local_cache_info_get: the local over-limit cache gauges of
 * limiter.localCacheStats (src/limiter/local_cache_stats.go:20-43):
 * lookup_count = Get calls (one per descriptor with a limit while the local cache
 * is enabled, fixed_cache_impl.go:57-67), hit_count, miss_count, and
 * entry_count = keys whose local-cache TTL has not passed at `now`. Counts are
 * cumulative since rl_create over the single-GPU batch path (rl_do_limit*,
 * rl_do_limit_requests). freecache's eviction/overwrite gauges have no
 * counterpart: entries live in the table's window records and are never evicted. */
typedef struct rl_local_cache_info {
  uint64_t entry_count;
  uint64_t lookup_count;
  uint64_t hit_count;
  uint64_t miss_count;
} rl_local_cache_info;
int rl_local_cache_info_get(rl_ctx* ctx, int64_t now, rl_local_cache_info* info);

/* Table snapshot / restore (Redis RDB-style restart): an exact image of the
 * counter table, the history log's written entries and append counters, the
 * long-stem arena, the local-cache state and the sweep time floor.
 * rl_snapshot_size gives the bytes rl_snapshot_save writes into `host`;
 * rl_snapshot_load accepts an image from a ctx with the same table_slots and
 * history_entries and an arena at least as large, whose live slots carry a
 * valid unit and long-stem arena offset (RL_E_INVALID otherwise). Both order
 * after every submitted batch. */
int rl_snapshot_size(rl_ctx* ctx, uint64_t* bytes);
int rl_snapshot_save(rl_ctx* ctx, void* host, uint64_t bytes);
int rl_snapshot_load(rl_ctx* ctx, const void* host, uint64_t bytes);

/* ---- Export / import of live counters (resize, reshard, re-key) -------------
 * A snapshot is an exact image: it loads only into a ctx of the same shape and
 * hash key. rl_export_range turns the live state into portable records, one
 * per Redis key (stem, unit, window start), and rl_import writes such records
 * into ANY ctx: other table_slots, history_entries, hash_seed or n_shards (the
 * Redis side of the reference: keys can be scanned, dumped and migrated, and a
 * cluster reshards under load, src/redis/driver_impl.go:108-126).
 *
 * rl_export_range orders after every submitted batch and is read-only. It
 * emits every window record of every live slot in [slot_begin, slot_end)
 * (clamped to shard_slots) of shard `shard`: the slot's newest window and the
 * newest version of each older window on its history chain. The records of one
 * (stem, unit) are contiguous, oldest window first; the order between keys is
 * unspecified. A slot is a key, so ranges that tile [0, shard_slots) yield
 * every key exactly once. Where a key's chain ends in an entry the log
 * overwrote or refused, its oldest emitted record carries RL_REC_CHAIN_LOST:
 * older windows may have had records (a request for one is RL_E_TIME, before
 * and after a move). out == NULL: only *info is filled (sizing). An `out` too
 * small for the range (records, or stem bytes, or a range holding 4 GiB of
 * stems or more: stem_off is 32-bit per call) gives RL_E_CAPACITY with
 * info->records / info->stem_bytes = what the range needs, and writes nothing.
 * Not on a ctx that joined a communicator (RL_E_INVALID).
 *
 * rl_import performs, per record, a raw SET of that one (stem, unit, window)
 * record: count, expire and lc verbatim (no clock, no fan-out to the records
 * of other units: the export carries those separately). in->n <= max_batch and
 * the stem bytes <= max_stem_bytes (RL_E_CAPACITY); a unit outside 1..4, a ws
 * that is no multiple of the unit's divider or above 2^32 - 172801, an empty
 * stem or one over 65535 bytes, or bad offsets give RL_E_INVALID and leave the
 * table untouched. Records of one key arrive oldest first (over one or several
 * calls): each newer window becomes the key's newest and the previous one goes
 * to this ctx's history log under its own horizon. RL_REC_CHAIN_LOST on the
 * first record of a key this ctx does not hold yet ends the key's chain in a
 * lost entry; on a key it holds the flag is ignored and the record overwrites
 * that window. New keys claim slots (and arena space) as requests do
 * (RL_E_TABLE_FULL / RL_E_ARENA_FULL). A multi-shard ctx routes the records to
 * their owners on the host. The sweep floor, the local-cache gauges and the
 * batches / decisions counters are left alone. */
#define RL_REC_CHAIN_LOST 0x1u
typedef struct rl_records {      /* host memory; one record per (stem, unit, window) */
  uint32_t n;          /* export: in = capacity in records, out = records written; import: records */
  uint32_t reserved;
  uint64_t stem_cap;   /* export: capacity of stem_bytes (import: ignored) */
  uint8_t* stem_bytes;
  uint32_t* stem_off;  /* n + 1, stem_off[0] == 0 */
  uint8_t* unit;       /* rl_unit */
  uint8_t* flags;      /* RL_REC_* */
  uint32_t* ws;        /* window start (the Redis key's suffix) */
  uint32_t* count;     /* INCRBY value */
  uint32_t* expire;    /* key live while now <= expire */
  uint32_t* lc;        /* local over-limit cache entry live while now < lc (0: none) */
} rl_records;
typedef struct rl_export_info {
  uint64_t shard_slots;  /* slots of this shard's table (the scan's upper bound) */
  uint64_t records, stem_bytes;  /* what the range holds (on RL_E_CAPACITY: what it needs) */
  uint64_t keys;         /* live (stem, unit) slots in the range */
  uint64_t chains_lost;  /* keys whose history chain ended at an overwritten or refused entry */
  int64_t time_floor;    /* the ctx's sweep floor */
} rl_export_info;
int rl_export_range(rl_ctx* ctx, uint32_t shard, uint64_t slot_begin, uint64_t slot_end, rl_records* out,
                    rl_export_info* info);
int rl_import(rl_ctx* ctx, const rl_records* in);

/* ---- Keyed read of counters (Redis GET + TTL, without counting a hit) --------
 * rl_lookup answers, per key, what a DoLimit descriptor with that (stem, unit)
 * and clock would read before its INCRBY. Key i is the Redis key
 * stem ‖ decimal((now/div)*div) in the store its unit selects under
 * per_second_split: found / count are what GET returns (the key is not found
 * once now > expire), expire gives the TTL (expire - now), and lc is the local
 * over-limit cache entry's expiry where IsOverLimitWithLocalCache would hit
 * (local cache enabled and now < lc), else 0. A stem counted under several
 * units shares Redis keys between its unit slots where their windows coincide:
 * the count is the first record of the window, in unit order, that is live at
 * now and in the same store; lc any such record's live entry.
 *
 * status[i]: RL_OK; RL_E_INVALID for a unit outside 1..4, an empty stem or one
 * over 65535 bytes; RL_E_TIME exactly where a request with that key and clock
 * is answered RL_E_TIME (clock outside [0, 2^32 - 172801] or below the sweep
 * floor; a history chain that breaks before the window is ruled out; a window
 * further back than the history proves). A failed key's other outputs are 0.
 *
 * Strictly read-only: no slot or arena space is claimed, nothing is appended,
 * no flag is set, and neither rl_table_info nor the local-cache gauges move.
 * Orders after every submitted batch; synchronous. A multi-shard ctx routes
 * the keys to their owners on the host and scatters the answers back. Whole-
 * call failures write nothing: null pointers or bad offsets (stem_off[0] != 0,
 * decreasing) RL_E_INVALID; n > max_batch or stem bytes > max_stem_bytes
 * RL_E_CAPACITY; a ctx that joined a communicator RL_E_INVALID. n == 0: RL_OK. */
typedef struct rl_keys {          /* host memory */
  uint32_t n, reserved;
  const uint8_t* stem_bytes;
  const uint32_t* stem_off;       /* n + 1, stem_off[0] == 0 */
  const uint8_t* unit;            /* [n] rl_unit */
  const int64_t* now;             /* [n] the clock the key is read at */
} rl_keys;
typedef struct rl_key_state {     /* host memory, same order */
  uint8_t* status;                /* [n] RL_OK / RL_E_INVALID / RL_E_TIME */
  uint8_t* found;                 /* [n] 1: the Redis key exists at now */
  uint32_t* count;                /* [n] its value (0 when !found) */
  uint32_t* expire;               /* [n] live while now <= expire (0 when !found) */
  uint32_t* lc;                   /* [n] local over-limit cache entry's expiry if now < lc, else 0 */
} rl_key_state;
int rl_lookup(rl_ctx* ctx, const rl_keys* in, rl_key_state* out);

/* ---- The busiest and the currently blocked keys (redis-cli --hotkeys, SCAN) --
 * rl_hot_keys answers "which keys have the largest counters in the window the
 * clock `now` falls in" and, with RL_HOT_BLOCKED, "which keys is the local
 * over-limit cache rejecting at `now`", without moving the table to the host:
 * one scan of the slots on the device, a selection there, k records back.
 *
 * It is defined against the export. A record matches when it is the record
 * rl_export_range emits last for its key (the key's newest window) and
 *   its unit is in unit_mask (0: every unit),
 *   ws == now - now % div(unit),
 *   now <= expire,
 *   count >= min_count, and
 *   with RL_HOT_BLOCKED, now < lc.
 * A key whose window at `now` is no longer its newest (the clock ran back:
 * that window lives in the history log) is NOT reported; the scan never walks
 * the log.
 *
 * min(k, matched) records come back in `out` (the export's rl_records: n and
 * stem_cap are the capacities on entry, n the records written on return,
 * stem_off[n] the stem bytes written; flags are 0): every matching record
 * with count > info->threshold, and for the rest records with count ==
 * threshold (which of the tied ones is unspecified). Order: count descending,
 * ties by stem bytes ascending (memcmp, the shorter first), then by unit.
 * info->above counts the returned records above the threshold (0 when none
 * is returned). k == 0: only *info (out may be NULL).
 *
 * A failed call writes nothing to `out`. RL_E_INVALID: a null q or info,
 * unknown flags, a unit_mask bit outside 1..4, RL_HOT_BLOCKED on a ctx without
 * local cache, out == NULL (or a null array in it) with k > 0, a ctx that
 * joined a communicator. RL_E_CAPACITY: k > max_batch; or out->n / stem_cap
 * (or the 32-bit stem offsets) too small for the result: *info is then filled
 * (min(k, matched) records are needed, of at most 65535 stem bytes each).
 * RL_E_TIME: now outside [0, 2^32 - 172801] or below the sweep floor.
 *
 * Orders after every submitted batch, is synchronous (it holds the batch
 * pipeline for its duration, like the export) and strictly read-only, like
 * rl_lookup: no slot, arena, flag, log entry, rl_table_info field or gauge
 * moves. On a multi-shard ctx every shard selects its own top k on its own
 * device and the host merges them; slots, matched and hits are summed,
 * threshold and above describe the merged answer. */
#define RL_HOT_BLOCKED 0x1u   /* only keys whose local over-limit cache entry is live: now < lc */
typedef struct rl_hot_query {
  int64_t  now;        /* the clock the table is read at */
  uint32_t k;          /* records wanted, 0..max_batch; 0: only *info */
  uint32_t min_count;  /* count >= min_count */
  uint32_t unit_mask;  /* bit u (1..4) selects rl_unit u; 0 = every unit */
  uint32_t flags;      /* RL_HOT_* */
} rl_hot_query;
typedef struct rl_hot_info {
  uint64_t slots;      /* slots scanned (summed over shards) */
  uint64_t matched;    /* records that satisfy the query */
  uint64_t hits;       /* sum of their counts */
  uint64_t above;      /* of them, with count > threshold */
  uint32_t threshold;  /* count of the last record returned (0: none returned) */
  uint32_t reserved;
  int64_t  time_floor; /* the ctx's sweep floor */
} rl_hot_info;
int rl_hot_keys(rl_ctx* ctx, const rl_hot_query* q, rl_records* out, rl_hot_info* info);

/* ---- Grow or shrink the counter table in place (a Redis dict's rehash) -------
 * rl_resize gives every shard of the ctx a table of `table_slots` slots and
 * places every live key in it on the device: nothing crosses to the host, the
 * ctx, its threads' handles, its config trie, gauges and counters stay. The
 * answer to RL_E_TABLE_FULL that needs no second ctx (rl_export_range +
 * rl_import remain the tools for re-keying and resharding).
 *
 * Size: table_slots is the new per-shard slot count, a power of two as
 * rl_create accepts it, from 2 to 2^32 (a slot index is a 32-bit word of the
 * history log), else RL_E_INVALID. It may be larger than, smaller than or
 * equal to the current count; equal is a full rehash that drops every
 * tombstone.
 *
 * Ordering: the call orders after every submitted batch (it completes pending
 * second halves of the packed and wire paths, host-fed batches and the
 * progress ring, as rl_export_range does), is synchronous and holds the batch
 * pipeline for its duration. RL_E_INVALID on a ctx that joined a communicator.
 *
 * Preserved: every live key keeps its 64-B slot image verbatim (tag, length,
 * unit, flags including the exact-path flag, the newest window record, the
 * chain head, stem bytes or arena offset). The long-stem arena and the history
 * log keep their size and contents, but for the `slot` word of the entries on
 * live keys' chains, which is re-pointed at the key's new slot. Untouched:
 * history_entries, history_appended / _lost / _refused, the sweep floor, the
 * local-cache gauges, batches, decisions, the loaded config and the hash key.
 * After success rl_table_info.table_slots is the new count and tombstones is
 * 0; live_slots, exact_stems, history_slots and arena_bytes_used are as
 * before; rl_snapshot_size follows the new count, and a snapshot of the ctx
 * loads into a fresh ctx created with the new table_slots.
 *
 * A failed call leaves the ctx exactly as it was (the same slot array, the
 * same log bytes, the same info):
 *   RL_E_TABLE_FULL  some key finds no free slot within min(table_slots,
 *                    65536) slots of its new home (found by the placement on
 *                    the device; more live slots than table_slots fails early);
 *   RL_E_HIP         the new table cannot be allocated: the old and the new
 *                    table (and 4 bytes per old slot) coexist during the call;
 *   RL_E_INTERNAL    a live slot's tag is not what its stem hashes to.
 * The log is re-pointed only after every key of every shard has been placed.
 * (A device failure after that point, which no input can cause, is RL_E_HIP
 * and leaves the ctx unusable, like any failed kernel.)
 *
 * Multi-shard ctx: every shard resizes to table_slots on its own device,
 * concurrently; no shard changes unless all placed. *info (optional) is summed
 * over the shards, longest_probe the maximum. */
typedef struct rl_resize_info {
  uint64_t slots_before, slots_after;   /* per call: summed over shards */
  uint64_t keys;                        /* live (stem, unit) slots placed in the new table */
  uint64_t tombstones_dropped;          /* tombstones of the old table (the new one has none) */
  uint64_t log_entries_relinked;        /* history-log entries re-pointed at their key's new slot */
  uint32_t longest_probe;               /* largest home-to-slot distance in the new table */
  uint32_t reserved;
} rl_resize_info;
int rl_resize(rl_ctx* ctx, uint64_t table_slots, rl_resize_info* info /* may be NULL */);

/* ---- Resize the history log in place ------------------------------------------
 * rl_resize_history rebuilds every shard's history log at another size, on the
 * device, from the live chains only: the answer to a growing
 * rl_table_info.history_lost or history_refused ("size history_entries up")
 * that needs no second ctx, the way to give the log's memory back, and the
 * log's only cleaner (rl_sweep and rl_forget leave a dead key's entries to be
 * overwritten; a ring full of unreachable entries wraps onto live ones just as
 * soon as a full one).
 *
 * Size: history_entries is rounded exactly as rl_create rounds it: per
 * partition (64 of them) a power of two, at least max(history_entries / 64,
 * max_batch / 16, 1024) and at most 2^25. 0, or more than 2^31, is
 * RL_E_INVALID. The new size may be larger than, smaller than or equal to the
 * current one; equal is a compaction that drops every unreachable entry, as an
 * equal rl_resize drops every tombstone.
 *
 * Ordering: as rl_resize. The call orders after every submitted batch, is
 * synchronous and holds the batch pipeline for its duration. RL_E_INVALID on a
 * ctx that joined a communicator.
 *
 * Preserved: for every live key with a chain, the entries that a lookup's walk
 * accepts from the chain's head (owner slot and tag, non-increasing append
 * time, a position inside its partition, no cycle, at most 65536 hops) are
 * copied, window records verbatim, every version of every window, in the same
 * order. A chain that ended cleanly ends cleanly; a chain that the log had cut
 * (an overwritten entry, a refused append) ends in the same place and its
 * lookups keep answering RL_E_TIME, a key whose head entry itself was lost
 * included. So every rl_do_limit*, rl_lookup, rl_export_range, rl_scan and
 * rl_sweep afterwards sees the same records for every key and ends the same
 * way: no answer changes. Entries that no live chain reaches are gone.
 * Untouched: the table, the arena, history_lost / _refused, the sweep floor,
 * the gauges, batches, decisions, the config and the hash key;
 * rl_table_info.history_appended does not drop. After success
 * rl_table_info.history_entries is the new size, rl_snapshot_size follows it,
 * and a snapshot of the ctx loads into a fresh ctx created with the new
 * history_entries (a snapshot taken before the call is refused, as any
 * snapshot of another log geometry is).
 *
 * A failed call leaves the ctx exactly as it was (the same log bytes, the same
 * slots, the same info):
 *   RL_E_CAPACITY  some partition of the new log was asked for more entries
 *                  than it holds (found by the placement on the device, which
 *                  never writes past a partition): choose a larger size;
 *   RL_E_HIP       the new log cannot be allocated: the old log, the new log
 *                  and 4 bytes per table slot coexist during the call.
 * The slots' chain heads are stored only after every shard has placed. (A
 * device failure after that point, which no input can cause, is RL_E_HIP and
 * leaves the ctx unusable, like any failed kernel.)
 *
 * Multi-shard ctx: every shard rebuilds its log at history_entries on its own
 * device, concurrently; no shard changes unless all placed. *info (optional)
 * is summed over the shards, longest_chain and fill_max the maxima. */
typedef struct rl_history_resize_info {
  uint64_t entries_before, entries_after;  /* the log's capacity: summed over shards */
  uint64_t written_before;                 /* entries the old log held: sum of min(append counter, partition size) */
  uint64_t entries_kept;                   /* entries copied: those on live keys' chains */
  uint64_t entries_dropped;                /* written_before - entries_kept */
  uint64_t chains;                         /* live keys with a chain */
  uint64_t chains_lost;                    /* of them, chains that end in a lost entry afterwards (as before) */
  uint64_t fill_max;                       /* most entries placed in one partition (of entries_after / 64 per shard) */
  uint32_t longest_chain;                  /* entries */
  uint32_t reserved;
} rl_history_resize_info;
int rl_resize_history(rl_ctx* ctx, uint64_t history_entries, rl_history_resize_info* info /* may be NULL */);

/* ---- Resize the long-stem arena in place --------------------------------------
 * rl_resize_arena gives every shard a long-stem arena (and the spare one that
 * rl_sweep compacts into) of arena_bytes: the answer to RL_E_ARENA_FULL that
 * needs no second ctx, and the way to give the arena's memory back.
 * arena_bytes must be a non-zero multiple of 16 of at most 2^36 (slots store
 * 32-bit offsets in 16-B units), else RL_E_INVALID; and at least the bytes in
 * use (rl_table_info.arena_bytes_used), else RL_E_ARENA_FULL and nothing
 * changes: run rl_sweep first, it compacts. The used bytes are copied device
 * to device and offsets do not change, so no slot is touched. Ordering as
 * rl_resize; the old and the new pair of arenas coexist during the call
 * (RL_E_HIP if the new pair cannot be allocated, the ctx as it was).
 * Multi-shard ctx: every shard does this, all or none. RL_E_INVALID on a ctx
 * that joined a communicator. */
int rl_resize_arena(rl_ctx* ctx, uint64_t arena_bytes);

/* ---- Delete keys by stem or by stem prefix (Redis DEL, SCAN MATCH + DEL) ------
 * rl_forget removes stems from the table on the device: the tenant that a
 * misconfigured limit blocked, the old window's count after a limit was
 * raised, a decommissioned domain. Without it a key leaves the table only
 * when every one of its windows and its local-cache entry has expired and a
 * sweep sees that.
 *
 * What is removed: a stem is removed whole, every unit slot it has, and with
 * each slot its newest window, its chain of older windows and its local
 * over-limit cache entries. Each removed slot gets tag = TAG_TOMB and ring =
 * LOG_NONE, exactly what rl_sweep's eviction leaves behind; its log entries
 * are left to be overwritten. In Redis terms: DEL of every key
 * stem ‖ decimal(ws) in both stores, plus the freecache entries of those keys.
 * There is deliberately no per-unit or per-window deletion: under the alias
 * rule unit slots of one stem stand for the same Redis key where
 * their windows coincide, and a partial delete would leave the key alive
 * through a sibling. Afterwards a request or rl_lookup for the stem behaves
 * as for a stem never seen: not found, count 0, no local-cache hit, a fresh
 * slot on the next hit.
 *
 * Keyed mode (no RL_FORGET_PREFIX): entry i is a whole stem, removed[i] the
 * number of its unit slots removed (0..4, 0 if absent). A stem given twice is
 * counted once, under either entry. Whole-call failures write nothing: a null
 * `in` (or array in it), bad offsets (stem_off[0] != 0, decreasing), unknown
 * flags, an empty stem or one over 65535 bytes RL_E_INVALID; n > max_batch or
 * stem bytes > max_stem_bytes RL_E_CAPACITY.
 *
 * Prefix mode (RL_FORGET_PREFIX): every entry is a stem prefix. A live slot
 * matches entry i when its stem is at least as long as the prefix and begins
 * with the prefix's bytes; the slot is counted under the lowest matching i.
 * One scan of the table serves all prefixes of the call. Whole-call failures,
 * beside the keyed mode's RL_E_INVALID ones: an empty prefix RL_E_INVALID
 * (there is no "flush everything"); n > RL_FORGET_PREFIX_MAX or their bytes >
 * RL_FORGET_PREFIX_BYTES RL_E_CAPACITY. Prefixes are bytes, not descriptor
 * entries: the reference's key format (domain_key_value_...) makes "a_" a
 * prefix of both domain "a" and domain "a_b", exactly as a Redis
 * SCAN MATCH a_* would see it.
 *
 * RL_FORGET_DRY_RUN: the same removed[] and *info as the real call would give
 * at that moment (with a stem listed more than once: the same sums); no byte
 * of the ctx changes.
 *
 * Ordering: the call orders after every submitted batch (it completes pending
 * second halves of the packed and wire paths, host-fed batches and the
 * progress ring, as rl_export_range and rl_resize do), is synchronous and
 * holds the batch pipeline for its duration.
 *
 * Untouched: the sweep floor, history_appended / _lost / _refused, batches,
 * decisions, the loaded config, the override-rule table and the local-cache
 * hit / miss counters. rl_table_info.live_slots drops by info->keys and
 * tombstones rises by the same amount (exact_stems and history_slots by the
 * removed slots that were flagged / had a chain); the slots become empty again
 * at the next rl_sweep under its reclamation rule, and the arena's bytes come
 * back at that sweep's compaction.
 *
 * A multi-shard ctx routes keyed stems to their owners on the host and
 * scatters removed[] back, like rl_lookup; prefixes go to every shard
 * concurrently, removed[] and *info summed. The whole call is checked before
 * any shard changes anything. RL_E_INVALID on a ctx that joined a
 * communicator. n == 0: RL_OK, *info zero. */
#define RL_FORGET_PREFIX  0x1u   /* every entry is a stem prefix, not a whole stem */
#define RL_FORGET_DRY_RUN 0x2u   /* select and count, change nothing */
#define RL_FORGET_PREFIX_MAX   64u    /* prefixes per call */
#define RL_FORGET_PREFIX_BYTES 4096u  /* their bytes per call */
typedef struct rl_stems {        /* host memory */
  uint32_t n, flags;             /* RL_FORGET_* */
  const uint8_t* stem_bytes;
  const uint32_t* stem_off;      /* n + 1, stem_off[0] == 0 */
} rl_stems;
typedef struct rl_forget_info {  /* 32 bytes */
  uint64_t slots_scanned;        /* prefix mode: slots read, summed over shards; keyed mode: 0 */
  uint64_t keys;                 /* (stem, unit) slots removed (dry run: that would be) */
  uint64_t keys_with_history;    /* of them, slots whose history chain was not empty */
  uint64_t arena_bytes;          /* long-stem arena bytes the next sweep's compaction gets back */
} rl_forget_info;
int rl_forget(rl_ctx* ctx, const rl_stems* in, uint32_t* removed /* [n] or NULL */,
              rl_forget_info* info /* may be NULL */);

/* ---- List keys by stem prefix, page by page (Redis SCAN MATCH + GET / TTL) -----
 * rl_scan is the read counterpart of rl_forget's prefix mode: "what does
 * tenant X hold right now". It selects on the device, returns only the
 * matching records, and can be resumed where the answer does not fit one
 * buffer. Like rl_hot_keys it is defined against the export.
 *
 * Which keys: a key is one live slot. It is selected when its unit is in
 * unit_mask (0: every unit) and either n_prefixes == 0 or its stem begins with
 * one of the prefixes: rl_forget's prefix rule, byte for byte (the stem is at
 * least as long as the prefix and its first bytes equal the prefix's). A key
 * is counted under the lowest matching prefix index; with n_prefixes == 0
 * by_prefix[0] takes everything.
 *
 * Which records: a selected key's records are those rl_export_range emits for
 * its slot, contiguous, oldest window first, count / expire / lc verbatim.
 * With RL_SCAN_NEWEST only the last of them (the slot's newest window) comes
 * back and the history log is never walked. With RL_SCAN_LIVE only records
 * with now <= expire come back (the Redis key exists at q->now). A selected
 * key without a record left after these filters is no key of the answer: it is
 * counted nowhere. A key whose chain walk broke carries RL_REC_CHAIN_LOST on
 * the first record emitted for it (never with RL_SCAN_NEWEST, which does not
 * walk); info->chains_lost counts such keys.
 *
 * One call stays inside one shard. It starts at *cur (all zero: the start) and
 * covers whole tiles of RL_SCAN_TILE slots, as many consecutive ones as fit
 * out->n records and out->stem_cap stem bytes (and 2^32 - 1 stem bytes: the
 * offsets are 32-bit); a shard's last tile may be short. It writes the records
 * of exactly the covered tiles, sets out->n and stem_off[0..n], and sets *cur
 * to the first slot not covered; at a shard's end the cursor becomes
 * {shard + 1, 0}. The scan is complete when cur->shard == n_shards; a call
 * with that cursor is RL_OK and returns the empty answer (out->n = 0, zero
 * sums). *info and by_prefix[] describe exactly the records of this call: sums
 * over the covered tiles. out == NULL covers the rest of the shard and only
 * counts. A first tile that does not fit gives RL_E_CAPACITY: nothing is
 * written, *cur is unchanged, and info->need_records / need_stem_bytes say what
 * that tile alone needs (the other fields of *info are zero but time_floor).
 *
 * Determinism: for an unchanged table and query, the concatenation of all
 * pages is the same byte sequence whatever capacities the calls were given. No
 * output position comes from an atomic race: positions are per-tile sums and
 * an in-workgroup scan.
 *
 * Cursor guarantee: a key that is in the table from the first page to the last
 * is returned exactly once (a key never changes its slot). Keys inserted or
 * evicted between pages may or may not appear. rl_resize and rl_snapshot_load
 * move keys between slots and so invalidate a cursor; the call cannot detect
 * that: start again from zero after either.
 *
 * Ordering: the call orders after every submitted batch (it completes pending
 * second halves of the packed and wire paths, host-fed batches and the
 * progress ring, as rl_export_range does), is synchronous and holds the batch
 * pipeline for its duration. Strictly read-only, like rl_lookup: no slot, arena
 * byte, flag, log entry, rl_table_info field or gauge moves.
 *
 * Failures, each writing nothing. RL_E_INVALID: a null q or cur; unknown
 * flags; non-zero reserved fields; a unit_mask bit outside 1..4; bad offsets
 * (prefix_off[0] != 0, decreasing) or a null prefix array with n_prefixes > 0;
 * an empty prefix; cur->slot no multiple of RL_SCAN_TILE or beyond the shard;
 * cur->shard > n_shards; a null array in a non-null out; a ctx that joined a
 * communicator. RL_E_CAPACITY: more than RL_FORGET_PREFIX_MAX prefixes or more
 * than RL_FORGET_PREFIX_BYTES bytes of them. RL_E_TIME, with RL_SCAN_LIVE: now
 * outside [0, 2^32 - 172801] or below the sweep floor. */
#define RL_SCAN_NEWEST 0x1u   /* only each key's newest window record; the history log is never walked */
#define RL_SCAN_LIVE   0x2u   /* only records whose Redis key exists at q->now: now <= expire */
#define RL_SCAN_TILE   1024u  /* a cursor advances in whole tiles of this many slots */
typedef struct rl_scan_query {
  uint32_t n_prefixes;          /* 0..RL_FORGET_PREFIX_MAX; 0: every key */
  uint32_t flags;               /* RL_SCAN_* */
  const uint8_t* prefix_bytes;  /* <= RL_FORGET_PREFIX_BYTES in all */
  const uint32_t* prefix_off;   /* n_prefixes + 1, prefix_off[0] == 0 */
  int64_t now;                  /* read with RL_SCAN_LIVE only */
  uint32_t unit_mask;           /* bit u (1..4) selects rl_unit u; 0 = every unit */
  uint32_t reserved;            /* zero */
} rl_scan_query;
typedef struct rl_scan_cursor { uint32_t shard, reserved; uint64_t slot; } rl_scan_cursor;  /* start: all zero */
typedef struct rl_scan_prefix_sum { uint64_t keys, records, hits; } rl_scan_prefix_sum;     /* hits: sum of the records' counts */
typedef struct rl_scan_info {
  uint64_t slots_scanned, keys, records, stem_bytes, chains_lost;
  uint64_t need_records, need_stem_bytes;  /* on RL_E_CAPACITY: what the first tile alone needs */
  int64_t time_floor;                      /* the ctx's sweep floor */
} rl_scan_info;
int rl_scan(rl_ctx* ctx, const rl_scan_query* q, rl_scan_cursor* cur /* in, out */,
            rl_records* out /* NULL: count only */, rl_scan_prefix_sum* by_prefix /* [max(n_prefixes, 1)] or NULL */,
            rl_scan_info* info /* may be NULL */);

/* Per-stage device timing (HIP events on the batch stream), for benchmarks.
 * rl_profile(ctx, k) with k >= 1 starts accumulating over every k-th batch,
 * the first sampled one being the k-th submitted after the call (1 = every
 * batch; the event markers and k_table's per-workgroup clock reads cost a
 * sampled batch a few microseconds, so a sparse sample keeps the timed
 * pipeline unchanged), 0 stops;
 * rl_profile_read fills ms[0..n) with
 * the summed milliseconds of the stages {prepare, sort, segment, table, finish}
 * and *batches with the number of batches timed (it synchronises), then resets
 * the sums. "segment" runs up to the start of k_table (the table stage's
 * wait for the previous batch included), "table" brackets the single k_table
 * launch (the keys seen once and the short runs: the bulk of the table work),
 * "finish" the rest (deferrals, long runs, outputs). With n > RL_NUM_STAGES,
 * ms[RL_NUM_STAGES] is k_table's own run time per batch, AVERAGED over every
 * batch since profiling started or was last read (not only the timed
 * sample): its first workgroup's start to its last workgroup's end on the
 * device's constant clock (the kernel duration rocprofv3 reports; no event is
 * recorded for it), where "table" also holds the launch's queueing behind the
 * other streams' kernels and the event markers' own cost. */
#define RL_NUM_STAGES 5
int rl_profile(rl_ctx* ctx, int enable);
int rl_profile_read(rl_ctx* ctx, double* ms, uint32_t n, uint64_t* batches);

#ifdef __cplusplus
}
#endif
#endif /* RATELIMIT_HIP_H */
