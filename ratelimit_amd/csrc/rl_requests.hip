// rl_requests.hip — the engine side of the request path: the calls that take
// raw requests instead of a ready DoLimit batch (rl_do_limit_requests[_verdict],
// rl_do_limit_requests_packed_async, rl_do_limit_wire[_respond]_async,
// rl_debug_verdict / rl_debug_respond, the override-rules calls). One layer for
// what they share: the carve of a device buffer (rl_request_layout.h), the
// views over it, the buffers that grow to the largest batch seen, the request
// slots and the stages of a pending batch, the lists of the output arrays. The
// kernels are rl_match.hip, rl_wire.hip and rl_resp.hip; the DoLimit batch
// path, which every request batch ends in, is rl_engine.hip (rl_engine_int.h).
// The order of HIP calls of every entry point is part of its behaviour: a
// helper here gathers calls that were adjacent, it never moves one across
// another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ratelimit_hip.h"
#include "rl_device.h"
#include "rl_kernels.h"
#include "rl_match.h"
#include "rl_engine.h"
#include "rl_engine_int.h"
#include "rl_request_layout.h"

using namespace rl;

namespace {

// ---- views over a carved buffer ---------------------------------------------

struct MatchViews {
  MatchBuf m;
  ReqOutDev ro;
};
MatchViews match_views(uint8_t* B, const rlreq::MatchPieces& p) {
  return {MatchBuf{(unsigned long long*)(B + p.v), (uint32_t*)(B + p.kind), (uint32_t*)(B + p.rpu),
                   (uint32_t*)(B + p.rule), (uint32_t*)(B + p.cnt)},
          ReqOutDev{B + p.code, (uint32_t*)(B + p.rem), (uint32_t*)(B + p.reset), B + p.match, (uint32_t*)(B + p.orule),
                    (uint32_t*)(B + p.orpu), B + p.ounit}};
}

// A batch's override arrays (all null: none).
struct OvArrays {
  uint8_t* ovf = nullptr;
  uint32_t* rpu = nullptr;
  uint8_t* unit = nullptr;
  uint32_t* rule = nullptr;
};
// The dense override arrays of a slot's mbuf: rpu and rule (4-byte aligned: n x 4 each), then flags and units.
OvArrays dense_ov(uint8_t* base, uint32_t n) {
  OvArrays o;
  o.rpu = (uint32_t*)base;
  o.rule = o.rpu + n;
  o.ovf = (uint8_t*)(o.rule + n);
  o.unit = o.ovf + n;
  return o;
}

// The match kernels' view of a request batch; each path passes its own sources.
ReqDev req_dev(uint32_t nq, uint32_t n, uint32_t ne, uint32_t dom_total, uint32_t desc_total, const uint8_t* dom,
               const uint32_t* dom_off, const uint32_t* hits, const uint32_t* req, const uint32_t* ent_first,
               const uint32_t* desc_off, const uint8_t* desc, const uint16_t* klen, const uint16_t* vlen,
               const OvArrays& ov) {
  ReqDev r;
  r.n_req = nq;
  r.n_desc = n;
  r.n_ent = ne;
  r.dom_total = dom_total;
  r.desc_total = desc_total;
  r.dom = dom;
  r.dom_off = dom_off;
  r.hits = hits;
  r.req = req;
  r.ent_first = ent_first;
  r.desc_off = desc_off;
  r.desc = desc;
  r.klen = klen;
  r.vlen = vlen;
  r.ovf = ov.ovf;
  r.ov_rpu = ov.rpu;
  r.ov_unit = ov.unit;
  r.ov_rule = ov.rule;
  return r;
}

// ---- copies, accumulating the first error -----------------------------------

// Host arrays into the pieces of a device buffer.
struct H2D {
  uint8_t* base;
  hipStream_t st;
  hipError_t e;
  void operator()(size_t off, const void* src, size_t bytes) {
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(base + off, src, bytes, hipMemcpyHostToDevice, st);
  }
};

// Device arrays into the caller's host arrays by copies on `st` (the
// synchronous calls; the pipelined ones: ToHostList, rl_engine_int.h).
struct D2H {
  hipStream_t st;
  hipError_t e = hipSuccess;
  void operator()(void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && dst && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  }
};

// The per-descriptor arrays of an rl_request_result (stats apart) and the
// per-request arrays of an rl_request_verdict with their device sources:
// copy(destination, source, bytes), one call per array.
template <typename Copy>
void result_arrays(const rl_request_result& out, const ReqOutDev& ro, uint32_t n, Copy& copy) {
  copy(out.code, ro.code, n);
  copy(out.limit_remaining, ro.rem, n * 4ull);
  copy(out.reset_s, ro.reset, n * 4ull);
  copy(out.match, ro.match, n);
  copy(out.rule_id, ro.rule, n * 4ull);
  copy(out.requests_per_unit, ro.rpu, n * 4ull);
  copy(out.unit, ro.unit, n);
}
template <typename Copy>
void verdict_arrays(const rl_request_verdict& v, const uint8_t* block, uint32_t nq, Copy& copy) {
  const VerdictLayout L = verdict_layout(nq);
  copy(v.overall_code, block + L.o_code, nq);
  copy(v.flags, block + L.o_flags, nq);
  copy(v.min_descriptor, block + L.o_min, nq * 4ull);
  copy(v.header_limit, block + L.o_limit, nq * 4ull);
  copy(v.header_remaining, block + L.o_rem, nq * 4ull);
  copy(v.header_reset_s, block + L.o_reset, nq * 4ull);
  copy(v.global_shadow, block + L.shadow, 8);
}

// A finished verdict block (device, verdict_layout(nq)) -> the caller's arrays.
hipError_t verdict_d2h(const uint8_t* block, uint32_t nq, rl_request_verdict* v, hipStream_t st) {
  D2H get{st};
  verdict_arrays(*v, block, nq, get);
  return get.e;
}

// The match stage's error bits -> the status and text of the batch.
struct Refusal {
  int code;
  const char* msg;
};
Refusal match_fail(uint32_t bits) {
  if (bits & MATCH_ERR_WIRE) return {RL_E_INVALID, "gpu: wire batch: a message's second walk left its counted share"};
  if (bits & MATCH_ERR_UNPACK)
    return {RL_E_INVALID, "gpu: malformed packed request batch (tile index or override list)"};
  if (bits & MATCH_ERR_REQ)
    return {RL_E_INVALID, "gpu: malformed request batch (request index or entry byte layout)"};
  return {RL_E_CAPACITY, "gpu: matched stems exceed max_stem_bytes"};
}

}  // namespace

namespace rl {

int eng_do_limit_requests(Engine* c, const rl_request_batch* in, rl_request_result* out, RequestsDoLimit run,
                          void* user, uint32_t opts, rl_request_verdict* verdict) {
  if (!c || !in || (!out && !verdict)) return set_err(c, RL_E_INVALID, "gpu: null argument");
  RQ_SETTLE(c);
  if (verdict && in->n_requests && !verdict->overall_code)
    return set_err(c, RL_E_INVALID, "gpu: rl_request_verdict without overall_code");
  if (verdict && (opts & ~RL_VERDICT_OPT_GLOBAL_SHADOW)) return set_err(c, RL_E_INVALID, "gpu: unknown verdict option");
  // checkServiceErr(snappedConfig != nil, ...) (ratelimit.go:106)
  if (!c->cfg_loaded) return set_err(c, RL_E_INVALID, "gpu: no rate limit configuration loaded");
  const uint32_t n = in->n_descriptors, nq = in->n_requests, ne = in->n_entries;
  if (n > c->cfg.max_batch || nq > c->cfg.max_requests || in->n_rules > c->cfg.max_rules)
    return set_err(c, RL_E_CAPACITY, "gpu: request batch exceeds configured max_batch/max_requests/max_rules");
  if (n && !nq) return set_err(c, RL_E_INVALID, "gpu: descriptors without requests");
  if (!in->domain_off || !in->entry_first || !in->desc_off || (nq && (!in->now || !in->hits)) ||
      (n && !in->req_idx) || (ne && (!in->key_len || !in->value_len)))
    return set_err(c, RL_E_INVALID, "gpu: null request batch array");
  const bool ovr = in->override_flags != nullptr;
  if (ovr && (!in->override_rpu || !in->override_unit || !in->override_rule))
    return set_err(c, RL_E_INVALID, "gpu: override_flags without override_rpu/unit/rule");
  if (in->entry_first[0] != 0 || in->entry_first[n] != ne || in->desc_off[0] != 0 || in->domain_off[0] != 0)
    return set_err(c, RL_E_INVALID, "gpu: request batch offsets must start at 0 and end at n_entries");
  const uint64_t dom_bytes = in->domain_off[nq], desc_bytes = in->desc_off[n];
  if ((dom_bytes && !in->domain_bytes) || (desc_bytes && !in->desc_bytes))
    return set_err(c, RL_E_INVALID, "gpu: null request byte array");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  // one device buffer, carved
  const size_t scan = n ? match_scan_bytes(n) : 0;
  rlreq::Carve cv;
  const size_t o_dom = cv.piece(dom_bytes), o_domoff = cv.piece((nq + 1) * 4ull), o_hits = cv.piece(nq * 4ull),
               o_req = cv.piece(n * 4ull), o_ent = cv.piece((n + 1) * 4ull), o_doff = cv.piece((n + 1) * 4ull),
               o_desc = cv.piece(desc_bytes), o_kl = cv.piece(ne * 2ull), o_vl = cv.piece(ne * 2ull),
               o_ovf = cv.piece(ovr ? n : 0), o_ovr = cv.piece(ovr ? n * 4ull : 0), o_ovu = cv.piece(ovr ? n : 0),
               o_ovrule = cv.piece(ovr ? n * 4ull : 0);
  const rlreq::MatchPieces mp = rlreq::match_pieces(cv, n, scan, verdict != nullptr, verdict_layout(nq).bytes);
  hipStream_t st = c->stream;
  HIPCHK(c, after_batches(c, st));
  if (cv.need > c->mbuf_cap) HIPCHK(c, hipStreamSynchronize(st));
  if (const int rc = grow(c, &c->mbuf, &c->mbuf_cap, cv.need, 0)) return rc;
  uint8_t* B = c->mbuf;
  H2D up{B, st, hipSuccess};
  up(o_dom, in->domain_bytes, dom_bytes);
  up(o_domoff, in->domain_off, (nq + 1) * 4ull);
  up(o_hits, in->hits, nq * 4ull);
  up(o_req, in->req_idx, n * 4ull);
  up(o_ent, in->entry_first, (n + 1) * 4ull);
  up(o_doff, in->desc_off, (n + 1) * 4ull);
  up(o_desc, in->desc_bytes, desc_bytes);
  up(o_kl, in->key_len, ne * 2ull);
  up(o_vl, in->value_len, ne * 2ull);
  OvArrays ov;
  if (ovr) {
    up(o_ovf, in->override_flags, n);
    up(o_ovr, in->override_rpu, n * 4ull);
    up(o_ovu, in->override_unit, n);
    up(o_ovrule, in->override_rule, n * 4ull);
    ov = OvArrays{B + o_ovf, (uint32_t*)(B + o_ovr), B + o_ovu, (uint32_t*)(B + o_ovrule)};
  }
  HIPCHK(c, up.e);
  if (nq) HIPCHK(c, hipMemcpyAsync(c->d_now, in->now, nq * 8ull, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(B + mp.cnt, 0, 16, st));
  const ReqDev r = req_dev(nq, n, ne, (uint32_t)dom_bytes, (uint32_t)desc_bytes, B + o_dom,
                           (const uint32_t*)(B + o_domoff), (const uint32_t*)(B + o_hits),
                           (const uint32_t*)(B + o_req), (const uint32_t*)(B + o_ent), (const uint32_t*)(B + o_doff),
                           B + o_desc, (const uint16_t*)(B + o_kl), (const uint16_t*)(B + o_vl), ov);
  const MatchViews mv = match_views(B, mp);
  // the matched descriptors become an ordinary DoLimit batch in the staging buffers
  PackOut po{c->d_stem, c->d_off, c->d_req, c->d_unit, c->d_flags, c->d_limit, c->d_hits, c->d_rule,
             c->cfg.max_stem_bytes};
  launch_match(c->cfg_dev, r, mv.m, po, B + mp.tmp, scan, st);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_match, B + mp.cnt, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (c->h_match[2] & (MATCH_ERR_REQ | MATCH_ERR_CAP)) {
    const Refusal f = match_fail(c->h_match[2]);
    return set_err(c, f.code, f.msg);
  }
  const uint32_t nm = n ? c->h_match[0] : 0;
  if (!n) {  // off[0] of the empty batch
    HIPCHK(c, hipMemsetAsync(c->d_off, 0, 4, st));
  }
  const rl_batch pb = staged_batch(nm, nq, in->n_rules, c->d_stem, c->d_off, c->d_now, c->d_req, c->d_unit,
                                   c->d_flags, c->d_limit, c->d_hits, c->d_rule);
  if (run) {
    rl_result dout{};
    dout.code = c->d_code;
    dout.limit_remaining = c->d_rem;
    dout.reset_s = c->d_reset;
    dout.stats = reinterpret_cast<uint64_t*>(c->d_stats);
    const int rc = run(user, &pb, &dout, st);
    if (rc) return rc;  // (the runner's own error report)
    HIPCHK(c, hipSetDevice(c->cfg.device));
  } else {
    BatchDev b = dev_view(c, &pb, c->cfg.max_stem_bytes);
    OutDev o{c->d_code, c->d_rem, c->d_reset, c->d_stats, nullptr};
    enqueue(c, b, o, 0, st, false);
  }
  launch_match_expand(r, mv.m, c->d_code, c->d_rem, c->d_reset, mv.ro, st);
  HIPCHK(c, hipGetLastError());
  uint8_t* vblock = B + mp.verdict;
  if (verdict && nq) {
    // the verdict reads the expanded answers where they lie
    const VerdictDev vd =
        verdict_view(nq, n, opts, r.req, mv.ro.match, mv.ro.code, mv.ro.rem, mv.ro.reset, mv.ro.rpu, vblock);
    HIPCHK(c, launch_verdict(vd, vblock, st));
  }
  if (out) {
    D2H get{st};
    result_arrays(*out, mv.ro, n, get);
    HIPCHK(c, get.e);
    if (in->n_rules && out->stats)
      HIPCHK(c, hipMemcpyAsync(out->stats, c->d_stats, (size_t)in->n_rules * RL_NUM_STATS * 8, hipMemcpyDeviceToHost, st));
  }
  c->batches++;
  c->decisions += nm;
  const int rc = collect(c);
  if (rc || !verdict) return rc;
  // copied only now that the batch is known good: a failed batch leaves *verdict alone
  if (nq) {
    HIPCHK(c, verdict_d2h(vblock, nq, verdict, st));
    HIPCHK(c, hipStreamSynchronize(st));
  } else if (verdict->global_shadow) {
    *verdict->global_shadow = 0;
  }
  return RL_OK;
}

// ---- packed request batches, pipelined (rl_do_limit_requests_packed_async) --

// The host checks only what the copy and the unpack's bounds rely on: sections
// inside buf, the index's first entry zero and its last the batch's sizes;
// every tile's own entry and the override list are checked on the device.
int eng_requests_packed_check(Engine* c, const rl_request_batch_packed* in, const rl_request_result* out, uint32_t opts,
                              const rl_request_verdict* verdict, uint32_t* tiles) {
  if (!c || !in || (!out && !verdict)) return set_err(c, RL_E_INVALID, "gpu: null argument");
  if (opts & ~RL_VERDICT_OPT_GLOBAL_SHADOW) return set_err(c, RL_E_INVALID, "gpu: unknown verdict option");
  if (!c->cfg_loaded) return set_err(c, RL_E_INVALID, "gpu: no rate limit configuration loaded");
  const rl_config& g = c->cfg;
  const uint32_t n = in->n_descriptors, nq = in->n_requests, ne = in->n_entries;
  if (n > g.max_batch || nq > g.max_requests || in->n_rules > g.max_rules)
    return set_err(c, RL_E_CAPACITY, "gpu: request batch exceeds configured max_batch/max_requests/max_rules");
  if (n && !nq) return set_err(c, RL_E_INVALID, "gpu: descriptors without requests");
  if (in->reserved) return set_err(c, RL_E_INVALID, "gpu: packed request batch: reserved field not zero");
  if (in->n_overrides > n) return set_err(c, RL_E_INVALID, "gpu: packed request batch: more overrides than descriptors");
  const uint32_t T = rlreq::tiles(nq, RL_REQUESTS_TILE);
  *tiles = T;
  const uint64_t B = in->buf_bytes;
  if (!in->buf) return set_err(c, RL_E_INVALID, "gpu: null argument");
  using rlreq::in_buf;
  if (!in_buf(B, in->index, 16ull * (T + 1)) || !in_buf(B, in->req, nq * 4ull) || !in_buf(B, in->now, nq * 4ull) ||
      !in_buf(B, in->hits, nq * 4ull) || !in_buf(B, in->desc, n * 2ull) || !in_buf(B, in->key_len, ne * 2ull) ||
      !in_buf(B, in->value_len, ne * 2ull) ||
      !in_buf(B, in->overrides, in->n_overrides * (uint64_t)sizeof(rl_request_override)) ||
      !in_buf(B, in->domain_bytes, 0) || !in_buf(B, in->entry_bytes, 0))
    return set_err(c, RL_E_INVALID, "gpu: packed request batch section outside buf or not 4-byte aligned");
  const uint32_t* ix = reinterpret_cast<const uint32_t*>(in->buf + in->index);
  const uint32_t* tot = ix + 4ull * T;
  if (!rlreq::index_ends_ok(ix, T, n, ne))
    return set_err(c, RL_E_INVALID, "gpu: packed request batch index does not start at zero or end at the batch's sizes");
  if (tot[3] > g.max_stem_bytes) return set_err(c, RL_E_CAPACITY, "gpu: request batch's entry bytes exceed max_stem_bytes");
  if (!in_buf(B, in->domain_bytes, tot[2]) || !in_buf(B, in->entry_bytes, tot[3]))
    return set_err(c, RL_E_INVALID, "gpu: packed request batch domain or entry bytes outside buf");
  return RL_OK;
}

void free_request_slots(Engine* c) {
  if (!c->rq) return;
  for (uint32_t j = 0; j < RL_REQUESTS_INFLIGHT; j++) {
    RequestSlot& s = c->rq[j];
    HostSlot& h = s.h;
    void* bufs[] = {h.stem, h.off, h.req, h.limit, h.hits, h.rule, h.now, h.unit, h.flags, h.code, h.rem,
                    h.reset, h.stats, h.cbuf, s.mbuf, s.wbuf};
    for (void* p : bufs)
      if (p) (void)hipFree(p);
    if (s.h_cnt) (void)hipHostFree(s.h_cnt);
    if (s.h_wcnt) (void)hipHostFree(s.h_wcnt);
    if (s.count_done) (void)hipEventDestroy(s.count_done);
    if (s.wire_done) (void)hipEventDestroy(s.wire_done);
    if (h.in_done) (void)hipEventDestroy(h.in_done);
  }
  if (c->rq_copy) (void)hipStreamDestroy(c->rq_copy);
  c->rq_copy = nullptr;
  delete[] c->rq;
  c->rq = nullptr;
  c->rq_head = c->rq_n = 0;
}

}  // namespace rl

namespace {

int ensure_request_slots(Engine* c) {
  if (c->rq) return RL_OK;
  const rl_config& g = c->cfg;
  c->rq = new RequestSlot[RL_REQUESTS_INFLIGHT];
  bool ok = rl_stream_create(&c->rq_copy, SR_HOSTCOPY) == hipSuccess;
  for (uint32_t j = 0; j < RL_REQUESTS_INFLIGHT; j++) {
    RequestSlot& s = c->rq[j];
    HostSlot& h = s.h;
    s.st = c->pipe[j % NBUF];
    ok = ok && dalloc(&h.stem, (size_t)g.max_stem_bytes + 64) == hipSuccess &&
         dalloc(&h.off, (size_t)g.max_batch + 1) == hipSuccess && dalloc(&h.req, g.max_batch) == hipSuccess &&
         dalloc(&h.limit, g.max_batch) == hipSuccess && dalloc(&h.hits, g.max_batch) == hipSuccess &&
         dalloc(&h.rule, g.max_batch) == hipSuccess && dalloc(&h.now, g.max_requests) == hipSuccess &&
         dalloc(&h.unit, g.max_batch) == hipSuccess && dalloc(&h.flags, g.max_batch) == hipSuccess &&
         dalloc(&h.code, g.max_batch) == hipSuccess && dalloc(&h.rem, g.max_batch) == hipSuccess &&
         dalloc(&h.reset, g.max_batch) == hipSuccess &&
         dalloc(&h.stats, (size_t)g.max_rules * RL_NUM_STATS) == hipSuccess &&
         hipHostMalloc((void**)&s.h_cnt, 16, hipHostMallocDefault) == hipSuccess &&
         hipEventCreateWithFlags(&s.count_done, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&h.in_done, hipEventDisableTiming) == hipSuccess;
  }
  if (!ok) {
    free_request_slots(c);
    return set_err(c, RL_E_HIP, "gpu: request slot allocation failed");
  }
  return RL_OK;
}

// The shared opening of the packed and the wire call: the slots; the oldest
// pending batches advanced (a full ring waits for the oldest one's count); the
// ring's next slot; its carved buffer (mbuf, or a wire batch's wbuf, of `need`
// bytes) and its copy of buf grown to the largest batch seen, behind the slot's
// previous batch; the batch's place in the progress ring (submitted now,
// complete when its second half is: the ring event is recorded then); the
// buffer's copy. The copy goes on a stream of its own: the slot's stream still
// runs its previous batch's second half, which reads nothing of cbuf (the first
// half did, and its count has arrived), and the batches' copies then follow
// each other on the link without waiting for any kernel.
int slot_submit_begin(Engine* c, bool wire, size_t need, const uint8_t* buf, uint64_t B, RequestSlot** slot) {
  int rc;
  if ((rc = ensure_request_slots(c))) return rc;
  if ((rc = eng_requests_advance(c, c->rq_n == RL_REQUESTS_INFLIGHT ? 1 : 0))) return rc;
  RequestSlot& s = c->rq[(c->rq_head + c->rq_n) % RL_REQUESTS_INFLIGHT];
  HostSlot& h = s.h;
  hipStream_t st = s.st;  // (after the slot's previous batch, in stream order)
  if (wire && !s.h_wcnt) {
    HIPCHK(c, hipHostMalloc((void**)&s.h_wcnt, 32, hipHostMallocDefault));
    HIPCHK(c, hipEventCreateWithFlags(&s.wire_done, hipEventDisableTiming));
  }
  uint8_t** carved = wire ? &s.wbuf : &s.mbuf;
  size_t* cap = wire ? &s.wbuf_cap : &s.mbuf_cap;
  if (need > *cap || B > h.cbuf_cap) HIPCHK(c, hipStreamSynchronize(st));  // the slot's previous batch
  if ((rc = grow(c, carved, cap, need, 0))) return rc;
  if ((rc = grow(c, &h.cbuf, &h.cbuf_cap, B, 64))) return rc;
  if (c->seq_sub - c->seq_done >= PROGRESS_RING) {
    HIPCHK(c, hipEventSynchronize(c->done_ring[c->seq_done % PROGRESS_RING]));
    c->seq_done++;
  }
  if (B) {
    HIPCHK(c, hipMemcpyAsync(h.cbuf, buf, B, hipMemcpyHostToDevice, c->rq_copy));
    HIPCHK(c, hipEventRecord(h.in_done, c->rq_copy));
    HIPCHK(c, hipStreamWaitEvent(st, h.in_done, 0));
  }
  *slot = &s;
  return RL_OK;
}

// The submitted batch in slot s becomes the ring's newest pending one.
void slot_pend(Engine* c, RequestSlot& s, uint32_t nq, uint32_t n_rules, uint32_t opts, const rl_request_result* out,
               rl_request_verdict* verdict) {
  s.nq = nq;
  s.n_rules = n_rules;
  s.opts = opts;
  s.seq = c->seq_sub++;
  s.has_out = out != nullptr;
  s.has_verdict = verdict != nullptr;
  if (out) s.out = *out;
  if (verdict) s.verdict = *verdict;
  if (verdict && !nq && verdict->global_shadow) *verdict->global_shadow = 0;
  c->rq_n++;
}

// The config match of the batch r in slot s on the slot's stream, the matched
// descriptors becoming an ordinary DoLimit batch in the slot's staging, and the
// matched count's way to the pinned words (by a kernel's stores: a DMA copy
// back would queue behind the next batch's input copy). The slot keeps the
// views for the second half.
int match_and_count(Engine* c, RequestSlot& s, const ReqDev& r, const MatchViews& mv, uint8_t* tmp, size_t scan) {
  HostSlot& h = s.h;
  PackOut po{h.stem, h.off, h.req, h.unit, h.flags, h.limit, h.hits, h.rule, c->cfg.max_stem_bytes};
  launch_match(c->cfg_dev, r, mv.m, po, tmp, scan, s.st);
  HIPCHK(c, hipGetLastError());
  ToHostList th(s.st);
  th(s.h_cnt, mv.m.count, 16);
  th.flush();
  HIPCHK(c, th.e);
  HIPCHK(c, hipEventRecord(s.count_done, s.st));
  s.n = r.n_desc;
  s.r = r;
  s.m = mv.m;
  s.ro = mv.ro;
  return RL_OK;
}

// The serializer's view of one batch: its answers, its verdict block and its staging (resp_layout at `stage`).
RespDev resp_view(uint32_t nq, uint32_t n, uint64_t bound, const uint32_t* req, const uint32_t* desc_first,
                  const uint8_t* status, const ReqOutDev& ro, uint8_t* vblock, uint8_t* stage) {
  const VerdictLayout V = verdict_layout(nq);
  const RespLayout L = resp_layout(nq, n, bound);
  RespDev r;
  r.n_req = nq;
  r.n_desc = n;
  r.cap = (uint32_t)L.cap;
  r.req = req;
  r.desc_first = desc_first;
  r.status = status;
  r.code = ro.code;
  r.rem = ro.rem;
  r.reset = ro.reset;
  r.match = ro.match;
  r.rpu = ro.rpu;
  r.unit = ro.unit;
  r.o_code = vblock + V.o_code;
  r.o_min = (const uint32_t*)(vblock + V.o_min);
  r.o_limit = (const uint32_t*)(vblock + V.o_limit);
  r.o_rem = (const uint32_t*)(vblock + V.o_rem);
  r.o_reset = (const uint32_t*)(vblock + V.o_reset);
  r.soff = (uint32_t*)(stage + L.soff);
  r.resp_off = (uint32_t*)(stage + L.resp_off);
  r.tmp = stage + L.tmp;
  r.tmp_bytes = L.tmp_bytes;
  r.bytes = stage + L.bytes;
  return r;
}

// The second half of the batch in slot s, whose count has arrived.
int request_second_half(Engine* c, RequestSlot& s) {
  HostSlot& h = s.h;
  const uint64_t seq = s.seq;
  // (a wire batch its middle stage refused has no count: rq_fail is set)
  const uint32_t n = s.n, nq = s.nq, bits = s.failed ? 0 : s.h_cnt[2];
  if (s.failed || bits) {
    // failed in the middle or the match stage: no second half, the table untouched;
    // its place in the progress ring completes with the work before it
    if (bits && !c->rq_fail) {
      const Refusal f = match_fail(bits);
      c->rq_fail = f.code;
      c->rq_fail_msg = f.msg;
    }
    HIPCHK(c, hipEventRecord(c->done_ring[seq % PROGRESS_RING], s.st));
    return RL_OK;
  }
  const uint32_t nm = n ? s.h_cnt[0] : 0;
  hipStream_t a = c->pipe[c->next];  // (the count is on the host: the first half is complete, nothing to wait for)
  if (!n) HIPCHK(c, hipMemsetAsync(h.off, 0, 4, a));  // off[0] of the empty batch
  const rl_batch pb =
      staged_batch(nm, nq, s.n_rules, h.stem, h.off, h.now, h.req, h.unit, h.flags, h.limit, h.hits, h.rule);
  BatchDev b = dev_view(c, &pb, c->cfg.max_stem_bytes);
  OutDev o{h.code, h.rem, h.reset, s.n_rules ? h.stats : nullptr, nullptr};
  const uint32_t k = enqueue(c, b, o, 0, nullptr, true);
  a = c->pipe[k];
  s.st = a;
  launch_match_expand(s.r, s.m, h.code, h.rem, h.reset, s.ro, a);
  HIPCHK(c, hipGetLastError());
  if ((s.has_verdict || s.has_resp) && nq) {
    const VerdictDev vd = verdict_view(nq, n, s.opts, s.r.req, s.ro.match, s.ro.code, s.ro.rem, s.ro.reset, s.ro.rpu,
                                       s.vblock);
    HIPCHK(c, launch_verdict(vd, s.vblock, a));
    if (s.wire) {  // a deferred or malformed request's entry is no answer
      launch_wire_code(s.w.status, s.vblock + verdict_layout(nq).o_code, nq, a);
      HIPCHK(c, hipGetLastError());
    }
  }
  ToHostList th(a);
  if (s.has_resp && nq) {  // the responses: serialized from the answers and the verdict where they lie
    const RespDev rd = resp_view(nq, n, s.resp_bound, s.r.req, s.w.desc_first, s.w.status, s.ro, s.vblock,
                                 s.mbuf + s.o_resp);
    HIPCHK(c, launch_respond(rd, s.fmt, a));
    launch_respond_to_host(rd, s.resp_dst, a);
    HIPCHK(c, hipGetLastError());
    th(s.resp.resp_off, rd.resp_off, (nq + 1) * 4ull);
  }
  if (s.wire) {
    th(s.wres.req_status, s.w.status, nq);
    th(s.wres.desc_first, s.w.desc_first, (nq + 1) * 4ull);
    th(s.wres.n_descriptors, s.w.cnt, 4);
  }
  if (s.has_out) {
    result_arrays(s.out, s.ro, n, th);
    if (s.n_rules) th(s.out.stats, h.stats, (size_t)s.n_rules * RL_NUM_STATS * 8);
  }
  if (s.has_verdict && nq) verdict_arrays(s.verdict, s.vblock, nq, th);
  th.flush();
  HIPCHK(c, th.e);
  HIPCHK(c, hipEventRecord(c->done_ring[seq % PROGRESS_RING], a));
  HIPCHK(c, hipGetLastError());
  c->batches++;
  c->decisions += nm;
  return RL_OK;
}

// The middle stage of the wire batch in slot s, whose count words have arrived:
// the capacity checks, the carve by the now-known sizes, k_wire_emit, the
// config match and the matched count's way to the host.
int request_middle(Engine* c, RequestSlot& s) {
  HostSlot& h = s.h;
  hipStream_t st = s.st;
  s.stage = 0;
  const uint32_t n = s.h_wcnt[0], ne = s.h_wcnt[1], dom_total = s.h_wcnt[2], ent_total = s.h_wcnt[3];
  const uint32_t bits = s.h_wcnt[4], nq = s.nq;
  const rl_config& g = c->cfg;
  Refusal f{0, nullptr};
  if (bits & WIRE_ERR_OFF)
    f = {RL_E_INVALID, "gpu: wire batch msg_off decreasing or past msgs_bytes"};
  else if ((bits & WIRE_ERR_SUM) || n > g.max_batch || (s.has_out && n > s.wres.desc_cap))
    f = {RL_E_CAPACITY, "gpu: wire batch has more descriptors than desc_cap / max_batch"};
  else if (ent_total > g.max_stem_bytes)
    f = {RL_E_CAPACITY, "gpu: request batch's entry bytes exceed max_stem_bytes"};
  // (the responses' length depends on the counters: the bound stands for it)
  s.resp_bound = s.has_resp ? rlresp::bound(nq, n, s.fmt) : 0;
  if (!f.code && s.has_resp && (s.resp_bound > s.resp.bytes_cap || s.resp_bound >= (1ull << 32)))
    f = {RL_E_CAPACITY, "gpu: wire batch's rl_response_bound exceeds bytes_cap or 32 bits"};
  if (f.code) {
    if (!c->rq_fail) {
      c->rq_fail = f.code;
      c->rq_fail_msg = f.msg;
    }
    s.failed = true;
    HIPCHK(c, hipEventRecord(s.count_done, st));
    return RL_OK;
  }
  const size_t scan = n ? match_scan_bytes(n) : 0;
  // the dense override arrays, as the packed path lays them out: only for a batch that carries overrides
  const bool has_ov = s.ov && s.h_wcnt[5] && n;
  const bool has_v = s.has_verdict || s.has_resp;
  rlreq::Carve cv;
  const size_t o_domoff = cv.piece((nq + 1) * 4ull), o_req = cv.piece(n * 4ull), o_ent = cv.piece((n + 1) * 4ull),
               o_doff = cv.piece((n + 1) * 4ull), o_hits = cv.piece(nq * 4ull), o_klen = cv.piece(ne * 2ull),
               o_vlen = cv.piece(ne * 2ull), o_dom = cv.piece(dom_total), o_desc = cv.piece(ent_total);
  const rlreq::MatchPieces mp = rlreq::match_pieces(cv, n, scan, has_v, verdict_layout(nq).bytes);
  const size_t o_ov = has_ov ? cv.piece(n * 10ull) : 0;
  s.o_resp = s.has_resp && nq ? cv.piece(resp_layout(nq, n, s.resp_bound).total) : 0;
  // (the count words are here: the slot's stream has nothing older in flight)
  if (cv.need > s.mbuf_cap) HIPCHK(c, hipStreamSynchronize(st));
  if (const int rc = grow(c, &s.mbuf, &s.mbuf_cap, cv.need, 0)) return rc;
  uint8_t* M = s.mbuf;
  HIPCHK(c, hipMemsetAsync(M + mp.cnt, 0, 16, st));
  const MatchViews mv = match_views(M, mp);
  const OvArrays ov = has_ov ? dense_ov(M + o_ov, n) : OvArrays{};
  WireOut wo;
  wo.tot = make_uint4(n, ne, dom_total, ent_total);
  wo.dom_off = (uint32_t*)(M + o_domoff);
  wo.hits = (uint32_t*)(M + o_hits);
  wo.now = h.now;
  wo.req = (uint32_t*)(M + o_req);
  wo.ent_first = (uint32_t*)(M + o_ent);
  wo.desc_off = (uint32_t*)(M + o_doff);
  wo.klen = (uint16_t*)(M + o_klen);
  wo.vlen = (uint16_t*)(M + o_vlen);
  wo.dom = M + o_dom;
  wo.desc = M + o_desc;
  wo.err = mv.m.count + 2;
  wo.ov_rpu = ov.rpu;
  wo.ov_rule = ov.rule;
  wo.ovf = ov.ovf;
  wo.ov_unit = ov.unit;
  if (has_ov) HIPCHK(c, hipMemsetAsync(M + o_ov, 0, n * 10ull, st));
  if (!nq) HIPCHK(c, hipMemsetAsync(wo.dom_off, 0, 4, st));
  launch_wire_emit(s.w, wo, st, has_ov ? &c->ov : nullptr);
  const ReqDev r = req_dev(nq, n, ne, dom_total, ent_total, wo.dom, wo.dom_off, wo.hits, wo.req, wo.ent_first,
                           wo.desc_off, wo.desc, wo.klen, wo.vlen, ov);
  s.vblock = has_v ? M + mp.verdict : nullptr;
  return match_and_count(c, s, r, mv, M + mp.tmp, scan);
}

}  // namespace

namespace rl {

int eng_requests_advance(Engine* c, uint32_t must) {
  if (!c->rq_n) return RL_OK;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  // wire batches whose count words have arrived: their middle stages, oldest first
  for (uint32_t i = 0; i < c->rq_n; i++) {
    RequestSlot& s = c->rq[(c->rq_head + i) % RL_REQUESTS_INFLIGHT];
    if (s.stage != 1) continue;
    const hipError_t e = hipEventQuery(s.wire_done);
    if (e == hipErrorNotReady) break;
    HIPCHK(c, e);
    if (const int rc = request_middle(c, s)) return rc;
  }
  while (c->rq_n) {
    RequestSlot& s = c->rq[c->rq_head];
    if (must) {
      if (s.stage == 1) {
        HIPCHK(c, hipEventSynchronize(s.wire_done));
        if (const int rc = request_middle(c, s)) return rc;
      }
      HIPCHK(c, hipEventSynchronize(s.count_done));
      must--;
    } else {
      if (s.stage == 1) break;
      const hipError_t e = hipEventQuery(s.count_done);
      if (e == hipErrorNotReady) break;
      HIPCHK(c, e);
    }
    c->rq_head = (c->rq_head + 1) % RL_REQUESTS_INFLIGHT;
    c->rq_n--;
    const int rc = request_second_half(c, s);
    if (rc) return rc;
  }
  return RL_OK;
}

int eng_do_limit_requests_packed_async(Engine* c, const rl_request_batch_packed* in, rl_request_result* out,
                                       uint32_t opts, rl_request_verdict* verdict) {
  uint32_t T = 0;
  int rc = eng_requests_packed_check(c, in, out, opts, verdict, &T);
  if (rc) return rc;
  const uint32_t n = in->n_descriptors, nq = in->n_requests, ne = in->n_entries, nov = in->n_overrides;
  const uint32_t* tot = reinterpret_cast<const uint32_t*>(in->buf + in->index) + 4ull * T;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const size_t scan = n ? match_scan_bytes(n) : 0;
  rlreq::Carve cv;
  const size_t o_domoff = cv.piece((nq + 1) * 4ull), o_req = cv.piece(n * 4ull), o_ent = cv.piece((n + 1) * 4ull),
               o_doff = cv.piece((n + 1) * 4ull), o_ov = cv.piece(nov ? n * 10ull : 0);
  const rlreq::MatchPieces mp = rlreq::match_pieces(cv, n, scan, verdict != nullptr, verdict_layout(nq).bytes);
  RequestSlot* slot = nullptr;
  if ((rc = slot_submit_begin(c, false, cv.need, in->buf, in->buf_bytes, &slot))) return rc;
  RequestSlot& s = *slot;
  HostSlot& h = s.h;
  hipStream_t st = s.st;
  uint8_t* M = s.mbuf;
  HIPCHK(c, hipMemsetAsync(M + mp.cnt, 0, 16, st));
  if (nov) HIPCHK(c, hipMemsetAsync(M + o_ov, 0, n * 10ull, st));
  const OvArrays ov = dense_ov(M + o_ov, n);
  const MatchViews mv = match_views(M, mp);
  launch_unpack_requests(*in, h.cbuf, (uint32_t*)(M + o_domoff), h.now, (uint32_t*)(M + o_req),
                         (uint32_t*)(M + o_ent), (uint32_t*)(M + o_doff), ov.ovf, ov.rpu, ov.unit, ov.rule,
                         mv.m.count + 2, st);
  const ReqDev r = req_dev(nq, n, ne, tot[2], tot[3], h.cbuf + in->domain_bytes, (const uint32_t*)(M + o_domoff),
                           (const uint32_t*)(h.cbuf + in->hits), (const uint32_t*)(M + o_req),
                           (const uint32_t*)(M + o_ent), (const uint32_t*)(M + o_doff), h.cbuf + in->entry_bytes,
                           (const uint16_t*)(h.cbuf + in->key_len), (const uint16_t*)(h.cbuf + in->value_len),
                           nov ? ov : OvArrays{});
  if ((rc = match_and_count(c, s, r, mv, M + mp.tmp, scan))) return rc;
  s.vblock = verdict ? M + mp.verdict : nullptr;
  s.stage = 0;
  s.wire = s.failed = s.has_resp = s.ov = false;
  slot_pend(c, s, nq, in->n_rules, opts, out, verdict);
  return RL_OK;
}

// ---- serialized payloads parsed on the device (rl_do_limit_wire_async) ------

int eng_do_limit_wire_async(Engine* c, const rl_wire_batch* in, rl_wire_result* wire, rl_request_result* out,
                            uint32_t opts, rl_request_verdict* verdict, const rl_response_format* fmt,
                            rl_response_batch* resp) {
  if (!c || !in || !wire || !wire->req_status || (!out && !verdict && !resp))
    return set_err(c, RL_E_INVALID, "gpu: null argument");
  rlresp::Format rf{};
  uint8_t* resp_dst = nullptr;
  if (resp) {
    if (!resp->bytes || !resp->resp_off) return set_err(c, RL_E_INVALID, "gpu: rl_response_batch without bytes or resp_off");
    if (!rlresp::format_from(fmt, &rf))
      return set_err(c, RL_E_INVALID, "gpu: rl_response_format: key over 64 bytes, NULL key with a length or reserved not zero");
  }
  if (opts & ~RL_VERDICT_OPT_GLOBAL_SHADOW) return set_err(c, RL_E_INVALID, "gpu: unknown verdict option");
  if (wire->reserved) return set_err(c, RL_E_INVALID, "gpu: rl_wire_result: reserved field not zero");
  if (!c->cfg_loaded) return set_err(c, RL_E_INVALID, "gpu: no rate limit configuration loaded");
  const rl_config& g = c->cfg;
  const uint32_t nq = in->n_requests;
  if (nq > g.max_requests || in->n_rules > g.max_rules)
    return set_err(c, RL_E_CAPACITY, "gpu: wire batch exceeds configured max_requests/max_rules");
  const uint64_t B = in->buf_bytes;
  if (!in->buf) return set_err(c, RL_E_INVALID, "gpu: null argument");
  using rlreq::in_buf;
  if (in->msgs_bytes > 0xFFFFFFFFull || !in_buf(B, in->msg_off, (nq + 1) * 4ull) || !in_buf(B, in->now, nq * 4ull) ||
      !in_buf(B, in->msgs, in->msgs_bytes))
    return set_err(c, RL_E_INVALID, "gpu: wire batch section outside buf or not 4-byte aligned");
  // (the two ends only: every offset between them is checked on the device)
  const uint32_t* mo = reinterpret_cast<const uint32_t*>(in->buf + in->msg_off);
  if (mo[0] || mo[nq] != in->msgs_bytes)
    return set_err(c, RL_E_INVALID, "gpu: wire batch msg_off does not start at zero or end at msgs_bytes");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (resp && resp->bytes_cap) {
    // the responses go out by a kernel's stores: both ends inside one page-locked allocation
    void* dp = nullptr;
    void* de = nullptr;
    if (hipHostGetDevicePointer(&dp, resp->bytes, 0) != hipSuccess || !dp ||
        hipHostGetDevicePointer(&de, resp->bytes + resp->bytes_cap - 1, 0) != hipSuccess ||
        (uint8_t*)de != (uint8_t*)dp + resp->bytes_cap - 1) {
      (void)hipGetLastError();  // (the failed lookup's sticky error: pageable memory)
      return set_err(c, RL_E_INVALID, "gpu: rl_response_batch.bytes is not page-locked over bytes_cap (rl_alloc_host)");
    }
    resp_dst = (uint8_t*)dp;
  }
  const uint32_t T = rlreq::tiles(nq, RL_WIRE_TILE);
  rlreq::Carve cv;
  const size_t o_reqw = cv.piece(nq * 16ull), o_tsum = cv.piece(T * 16ull), o_index = cv.piece((T + 1) * 16ull),
               o_cnt = cv.piece(32), o_status = cv.piece(nq), o_first = cv.piece((nq + 1) * 4ull),
               o_miss = c->ov_on ? cv.piece(nq * 4ull) : 0;
  RequestSlot* slot = nullptr;
  if (const int rc = slot_submit_begin(c, true, cv.need, in->buf, B, &slot)) return rc;
  RequestSlot& s = *slot;
  HostSlot& h = s.h;
  hipStream_t st = s.st;
  uint8_t* W = s.wbuf;
  WireDev w;
  w.n_req = nq;
  w.tiles = T;
  w.msgs_bytes = (uint32_t)in->msgs_bytes;
  w.msg_off = (const uint32_t*)(h.cbuf + in->msg_off);
  w.now32 = (const uint32_t*)(h.cbuf + in->now);
  w.msgs = h.cbuf + in->msgs;
  w.reqw = (uint4*)(W + o_reqw);
  w.tsum = (uint4*)(W + o_tsum);
  w.index = (uint4*)(W + o_index);
  w.cnt = (uint32_t*)(W + o_cnt);
  w.status = W + o_status;
  w.desc_first = (uint32_t*)(W + o_first);
  w.n_rules = in->n_rules;
  w.miss = c->ov_on ? (uint32_t*)(W + o_miss) : nullptr;
  HIPCHK(c, hipMemsetAsync(w.cnt, 0, 32, st));
  launch_wire_count(w, st, c->ov_on ? &c->ov : nullptr, c->ov_order, c->ov_ordered);
  if (c->ov_on && T) c->ov_ordered = true;
  HIPCHK(c, hipGetLastError());
  ToHostList th(st);
  th(s.h_wcnt, w.cnt, 32);
  th.flush();
  HIPCHK(c, th.e);
  HIPCHK(c, hipEventRecord(s.wire_done, st));
  s.stage = 1;
  s.wire = true;
  s.failed = false;
  s.ov = c->ov_on;
  s.w = w;
  s.wres = *wire;
  s.n = 0;
  s.has_resp = resp != nullptr;
  if (resp) {
    s.fmt = rf;
    s.resp = *resp;
    s.resp_dst = resp_dst;
    if (!nq) resp->resp_off[0] = 0;
  }
  slot_pend(c, s, nq, in->n_rules, opts, out, verdict);
  return RL_OK;
}

// ---- override stats keys interned on the device (rl_override_rules_enable) --

int eng_override_rules_enable(Engine* c, const rl_override_rules_config* cfg) {
  if (!c || !cfg) return set_err(c, RL_E_INVALID, "gpu: null argument");
  if (c->ov_on) return set_err(c, RL_E_INVALID, "gpu: rl_override_rules_enable: already enabled on this ctx");
  if (cfg->reserved[0] || cfg->reserved[1] || cfg->reserved[2] || cfg->reserved[3])
    return set_err(c, RL_E_INVALID, "gpu: rl_override_rules_config: reserved field not zero");
  if (!cfg->capacity || (uint64_t)cfg->first_rule + cfg->capacity > c->cfg.max_rules)
    return set_err(c, RL_E_INVALID, "gpu: rl_override_rules_config: capacity zero or first_rule + capacity > max_rules");
  RQ_SETTLE(c);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  // (offsets into the arena are 32-bit: it holds at most 4 GiB - 1)
  const uint64_t want = cfg->key_bytes ? cfg->key_bytes : 64ull * cfg->capacity;
  const uint32_t arena_cap = (uint32_t)std::min<uint64_t>(want, 0xFFFFFFFFull);
  uint64_t nslots = 64;
  while (nslots < 4ull * cfg->capacity) nslots *= 2;  // (a quarter full at the most: short probes)
  OvDev t{};
  hipEvent_t ev = nullptr;
  const bool ok = dalloc(&t.slots, nslots) == hipSuccess && dalloc(&t.koff, cfg->capacity) == hipSuccess &&
                  dalloc(&t.klen, cfg->capacity) == hipSuccess && dalloc(&t.arena, arena_cap) == hipSuccess &&
                  dalloc(&t.ctr, 2) == hipSuccess &&
                  hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess &&
                  hipMemsetAsync(t.slots, 0, nslots * 8, c->stream) == hipSuccess &&
                  hipMemsetAsync(t.ctr, 0, 16, c->stream) == hipSuccess &&
                  hipStreamSynchronize(c->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    for (void* p : {(void*)t.slots, (void*)t.koff, (void*)t.klen, (void*)t.arena, (void*)t.ctr})
      if (p) (void)hipFree(p);
    if (ev) (void)hipEventDestroy(ev);
    return set_err(c, RL_E_HIP, "gpu: rl_override_rules_enable: device allocation failed");
  }
  t.mask = (uint32_t)(nslots - 1);
  t.first_rule = cfg->first_rule;
  t.capacity = cfg->capacity;
  t.arena_cap = arena_cap;
  t.k0 = c->hk.k0;
  t.k1 = c->hk.k1;
  c->ov = t;
  c->ov_order = ev;
  c->ov_on = true;
  return RL_OK;
}

namespace {
// The table's counter words, after every submitted batch.
int ov_counters(Engine* c, unsigned long long* ctr) {
  RQ_SETTLE(c);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  hipStream_t st = c->stream;
  HIPCHK(c, after_batches(c, st));
  if (c->ov_ordered) HIPCHK(c, hipStreamWaitEvent(st, c->ov_order, 0));
  HIPCHK(c, hipMemcpyAsync(ctr, c->ov.ctr, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return RL_OK;
}
}  // namespace

int eng_override_rules_info_get(Engine* c, rl_override_rules_info* info) {
  if (!c || !info) return set_err(c, RL_E_INVALID, "gpu: null argument");
  if (!c->ov_on) return set_err(c, RL_E_INVALID, "gpu: override rules are not enabled on this ctx (rl_override_rules_enable)");
  unsigned long long ctr[2];
  if (const int rc = ov_counters(c, ctr)) return rc;
  rl_override_rules_info x{};
  x.first_rule = c->ov.first_rule;
  x.capacity = c->ov.capacity;
  x.rules = (uint32_t)(ctr[0] >> 32);
  x.key_bytes_used = (uint32_t)ctr[0];
  x.key_bytes_cap = c->ov.arena_cap;
  x.deferred_full = ctr[1];
  *info = x;
  return RL_OK;
}

int eng_override_rule_keys(Engine* c, uint32_t from_rule, uint32_t n, uint8_t* bytes, uint64_t cap, uint32_t* off,
                           uint64_t* needed) {
  if (!c || !off) return set_err(c, RL_E_INVALID, "gpu: null argument");
  if (!c->ov_on) return set_err(c, RL_E_INVALID, "gpu: override rules are not enabled on this ctx (rl_override_rules_enable)");
  unsigned long long ctr[2];
  if (const int rc = ov_counters(c, ctr)) return rc;
  const uint32_t rules = (uint32_t)(ctr[0] >> 32), first = c->ov.first_rule;
  if (from_rule < first || from_rule - first > rules || n > rules - (from_rule - first))
    return set_err(c, RL_E_INVALID, "gpu: rl_override_rule_keys: range outside the ids handed out");
  off[0] = 0;
  if (needed) *needed = 0;
  if (!n) return RL_OK;
  const uint32_t i0 = from_rule - first;
  std::vector<uint32_t> koff(n), klen(n);
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(koff.data(), c->ov.koff + i0, n * 4ull, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(klen.data(), c->ov.klen + i0, n * 4ull, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (koff[i] > c->ov.arena_cap || klen[i] > c->ov.arena_cap - koff[i])
      return set_err(c, RL_E_HIP, "gpu: rl_override_rule_keys: a key lies outside the arena");
    total += klen[i];
    off[i + 1] = (uint32_t)total;
  }
  if (needed) *needed = total;
  if (total > cap || total > 0xFFFFFFFFull || (total && !bytes))
    return set_err(c, RL_E_CAPACITY, "gpu: rl_override_rule_keys: the keys take " + std::to_string(total) + " bytes");
  // (ids are handed out with their bytes, in one step: consecutive ids lie next to each other unless
  // inserts raced; copied key by key all the same, the call is rare)
  for (uint32_t i = 0; i < n; i++)
    if (klen[i])
      HIPCHK(c, hipMemcpyAsync(bytes + off[i], c->ov.arena + koff[i], klen[i], hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return RL_OK;
}

// ---- the verdict and the serializer on explicit answers ----------------------
// (Each call owns one carved device buffer, freed when it returns.)

int eng_debug_respond(Engine* c, uint32_t nq, uint32_t n, const uint32_t* req_idx, const uint8_t* req_status,
                      const rl_request_result* ans, uint32_t opts, const rl_response_format* fmt,
                      rl_response_batch* resp) {
  if (!c || !resp || !resp->resp_off || !ans) return set_err(c, RL_E_INVALID, "gpu: null argument");
  RQ_SETTLE(c);
  if (opts & ~RL_VERDICT_OPT_GLOBAL_SHADOW) return set_err(c, RL_E_INVALID, "gpu: unknown verdict option");
  rlresp::Format rf{};
  if (!rlresp::format_from(fmt, &rf))
    return set_err(c, RL_E_INVALID, "gpu: rl_response_format: key over 64 bytes, NULL key with a length or reserved not zero");
  if (n > c->cfg.max_batch || nq > c->cfg.max_requests)
    return set_err(c, RL_E_CAPACITY, "gpu: verdict input exceeds configured max_batch/max_requests");
  if (n && (!req_idx || !ans->match || !ans->code || !ans->limit_remaining || !ans->reset_s ||
            !ans->requests_per_unit || !ans->unit))
    return set_err(c, RL_E_INVALID, "gpu: null answer array");
  std::vector<uint32_t> first((size_t)nq + 1, 0);
  for (uint32_t d = 0; d < n; d++) {
    if (req_idx[d] >= nq || (d && req_idx[d] < req_idx[d - 1]))
      return set_err(c, RL_E_INVALID, "gpu: req_idx must be non-decreasing and below n_requests");
    if (req_status && req_status[req_idx[d]] != RL_WIRE_OK)
      return set_err(c, RL_E_INVALID, "gpu: a deferred or malformed request has no descriptors");
    if (ans->reset_s[d] >= (1u << 21)) return set_err(c, RL_E_INVALID, "gpu: reset_s must be below 2^21");
    first[req_idx[d] + 1]++;
  }
  for (uint32_t q = 0; q < nq; q++) first[q + 1] += first[q];
  resp->resp_off[0] = 0;
  if (!nq) return RL_OK;
  const uint64_t bound = rlresp::bound(nq, n, rf);
  if (!resp->bytes) return set_err(c, RL_E_INVALID, "gpu: rl_response_batch without bytes or resp_off");
  if (bound > resp->bytes_cap || bound >= (1ull << 32))
    return set_err(c, RL_E_CAPACITY, "gpu: rl_response_bound exceeds bytes_cap or 32 bits");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const VerdictLayout vl = verdict_layout(nq);
  rlreq::Carve cv;
  const size_t o_req = cv.piece(n * 4ull), o_first = cv.piece((nq + 1) * 4ull), o_status = cv.piece(nq),
               o_match = cv.piece(n), o_code = cv.piece(n), o_rem = cv.piece(n * 4ull), o_reset = cv.piece(n * 4ull),
               o_rpu = cv.piece(n * 4ull), o_unit = cv.piece(n), o_verdict = cv.piece(vl.bytes),
               o_resp = cv.piece(resp_layout(nq, n, bound).total);
  DevBufs mem;
  uint8_t* B = nullptr;
  HIPCHK(c, mem.get(&B, cv.need));
  hipStream_t st = c->stream;
  H2D up{B, st, after_batches(c, st)};
  up(o_req, req_idx, n * 4ull);
  up(o_first, first.data(), (nq + 1) * 4ull);
  if (req_status) up(o_status, req_status, nq);
  up(o_match, ans->match, n);
  up(o_code, ans->code, n);
  up(o_rem, ans->limit_remaining, n * 4ull);
  up(o_reset, ans->reset_s, n * 4ull);
  up(o_rpu, ans->requests_per_unit, n * 4ull);
  up(o_unit, ans->unit, n);
  HIPCHK(c, up.e);
  const ReqOutDev ro{B + o_code, (uint32_t*)(B + o_rem), (uint32_t*)(B + o_reset), B + o_match, nullptr,
                     (uint32_t*)(B + o_rpu), B + o_unit};
  const VerdictDev vd = verdict_view(nq, n, opts, (const uint32_t*)(B + o_req), ro.match, ro.code, ro.rem, ro.reset,
                                     ro.rpu, B + o_verdict);
  HIPCHK(c, launch_verdict(vd, B + o_verdict, st));
  if (req_status) launch_wire_code(B + o_status, B + o_verdict + vl.o_code, nq, st);
  const RespDev rd = resp_view(nq, n, bound, (const uint32_t*)(B + o_req), (const uint32_t*)(B + o_first),
                               req_status ? B + o_status : nullptr, ro, B + o_verdict, B + o_resp);
  HIPCHK(c, launch_respond(rd, rf, st));
  HIPCHK(c, hipMemcpyAsync(resp->resp_off, rd.resp_off, (nq + 1) * 4ull, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const uint64_t total = std::min<uint64_t>(resp->resp_off[nq], bound);
  if (total) HIPCHK(c, hipMemcpyAsync(resp->bytes, rd.bytes, total, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return RL_OK;
}

int eng_debug_verdict(Engine* c, uint32_t nq, uint32_t n, const uint32_t* req_idx, const uint8_t* match,
                      const uint8_t* code, const uint32_t* limit_remaining, const uint32_t* reset_s,
                      const uint32_t* requests_per_unit, uint32_t opts, rl_request_verdict* verdict) {
  if (!c || !verdict) return set_err(c, RL_E_INVALID, "gpu: null argument");
  RQ_SETTLE(c);
  if (nq && !verdict->overall_code) return set_err(c, RL_E_INVALID, "gpu: rl_request_verdict without overall_code");
  if (opts & ~RL_VERDICT_OPT_GLOBAL_SHADOW) return set_err(c, RL_E_INVALID, "gpu: unknown verdict option");
  if (n > c->cfg.max_batch || nq > c->cfg.max_requests)
    return set_err(c, RL_E_CAPACITY, "gpu: verdict input exceeds configured max_batch/max_requests");
  if (n && (!req_idx || !match || !code || !limit_remaining || !reset_s || !requests_per_unit))
    return set_err(c, RL_E_INVALID, "gpu: null verdict input array");
  for (uint32_t d = 0; d < n; d++)
    if (req_idx[d] >= nq || (d && req_idx[d] < req_idx[d - 1]))
      return set_err(c, RL_E_INVALID, "gpu: req_idx must be non-decreasing and below n_requests");
  if (!nq) {
    if (verdict->global_shadow) *verdict->global_shadow = 0;
    return RL_OK;
  }
  HIPCHK(c, hipSetDevice(c->cfg.device));
  rlreq::Carve cv;
  const size_t o_req = cv.piece(n * 4ull), o_match = cv.piece(n), o_code = cv.piece(n), o_rem = cv.piece(n * 4ull),
               o_reset = cv.piece(n * 4ull), o_rpu = cv.piece(n * 4ull), o_verdict = cv.piece(verdict_layout(nq).bytes);
  DevBufs mem;
  uint8_t* B = nullptr;
  HIPCHK(c, mem.get(&B, cv.need));
  hipStream_t st = c->stream;
  H2D up{B, st, after_batches(c, st)};
  up(o_req, req_idx, n * 4ull);
  up(o_match, match, n);
  up(o_code, code, n);
  up(o_rem, limit_remaining, n * 4ull);
  up(o_reset, reset_s, n * 4ull);
  up(o_rpu, requests_per_unit, n * 4ull);
  HIPCHK(c, up.e);
  const VerdictDev vd = verdict_view(nq, n, opts, (const uint32_t*)(B + o_req), B + o_match, B + o_code,
                                     (const uint32_t*)(B + o_rem), (const uint32_t*)(B + o_reset),
                                     (const uint32_t*)(B + o_rpu), B + o_verdict);
  HIPCHK(c, launch_verdict(vd, B + o_verdict, st));
  HIPCHK(c, verdict_d2h(B + o_verdict, nq, verdict, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return RL_OK;
}

}  // namespace rl
