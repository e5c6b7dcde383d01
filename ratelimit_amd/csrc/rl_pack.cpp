// rl_pack.cpp — host packer: serialized
// envoy.service.ratelimit.v3.RateLimitRequest messages, as the gRPC server
// receives them, parsed straight into the rl_request_batch arrays of
// rl_do_limit_requests, so the host never builds per-descriptor objects.
//
// Wire format (proto3; go-control-plane v0.9.7 rls.proto / ratelimit.proto):
//   RateLimitRequest      1: domain (string)  2: descriptors (repeated message)  3: hits_addend (uint32)
//   RateLimitDescriptor   1: entries (repeated message)  2: limit (RateLimitOverride)
//   Entry                 1: key (string)  2: value (string)
//   RateLimitOverride     1: requests_per_unit (uint32)  2: unit (enum)
// Unknown fields are skipped by wire type; a truncated or malformed message
// fails the call with RL_E_INVALID. An override's stats key is
// descriptorKey(domain, descriptor) (src/config/config_impl.go:300-312),
// interned here to a dense rule id; rl_packer_rule_key names it for the caller's
// stats sink.
#include <stdint.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ratelimit_hip.h"
#include "rl_resp_emit.h"

namespace rlpack {

// A growable array of plain values that is never value-initialised (the
// packer writes every element it hands out) and keeps its storage across
// batches: after the first batches no call allocates.
template <typename T>
struct Buf {
  T* p = nullptr;
  size_t n = 0, cap = 0;
  ~Buf() { delete[] p; }
  void clear() { n = 0; }
  void reserve(size_t m) {
    if (m <= cap) return;
    size_t c = cap ? cap : 1024;
    while (c < m) c *= 2;
    T* q = new T[c];
    if (n) memcpy(q, p, n * sizeof(T));
    delete[] p;
    p = q;
    cap = c;
  }
  void push(T v) {
    if (n == cap) reserve(n + 1);
    p[n++] = v;
  }
  T* grow(size_t k) {  // k more elements, returned for writing
    reserve(n + k);
    T* r = p + n;
    n += k;
    return r;
  }
};

}  // namespace rlpack

using rlpack::Buf;

struct rl_packer {
  uint32_t first_rule;
  std::unordered_map<std::string, uint32_t> ids;
  std::vector<std::string> keys;
  std::string err;
  // the batch arrays (valid until the next rl_packer_pack)
  Buf<uint8_t> dom, desc, ovf, ovu;
  Buf<uint32_t> dom_off, hits, req, ent_first, desc_off, ovr, ovrule;
  Buf<int64_t> now;
  Buf<uint16_t> klen, vlen;
  std::vector<uint32_t> pend;  // descriptors of the current message whose override key waits for its domain
  std::string dkey;    // descriptorKey scratch
};

namespace {

struct Rd {
  const uint8_t* p;
  const uint8_t* e;
  bool ok = true;
  bool more() const { return ok && p < e; }
  uint64_t varint() {
    if (p < e && !(*p & 0x80)) return *p++;  // (one-byte tags and lengths: the common case)
    uint64_t v = 0;
    for (int s = 0; s < 64; s += 7) {
      if (p >= e) { ok = false; return 0; }
      const uint8_t b = *p++;
      v |= (uint64_t)(b & 0x7F) << s;
      if (!(b & 0x80)) return v;
    }
    ok = false;
    return 0;
  }
  // a length-delimited field's bytes
  Rd sub() {
    const uint64_t n = varint();
    if (!ok || n > (uint64_t)(e - p)) { ok = false; return Rd{p, p}; }
    Rd r{p, p + n};
    p += n;
    return r;
  }
  void skip(uint32_t wt) {
    if (wt == 0) varint();
    else if (wt == 1) { if (e - p < 8) ok = false; else p += 8; }
    else if (wt == 2) sub();
    else if (wt == 5) { if (e - p < 4) ok = false; else p += 4; }
    else ok = false;  // groups (3, 4) are not used by these messages
  }
};

// A field key of these messages: field numbers 1..3 only matter; 0 or one
// past 2^29 - 1 (the protobuf limit) makes the message malformed.
inline bool field_ok(uint64_t tag) { return (tag >> 3) != 0 && (tag >> 3) <= 0x1FFFFFFFull; }

// Small copies inline (entry keys and values are a few bytes): overlapping
// 8-byte moves instead of a libc call per field.
inline void copy_small(uint8_t* __restrict d, const uint8_t* __restrict s, size_t n) {
  if (n >= 8 && n <= 16) {
    uint64_t a, b;
    memcpy(&a, s, 8);
    memcpy(&b, s + n - 8, 8);
    memcpy(d, &a, 8);
    memcpy(d + n - 8, &b, 8);
  } else if (n > 16) {
    memcpy(d, s, n);
  } else {
    for (size_t i = 0; i < n; i++) d[i] = s[i];
  }
}

// The batch being written: raw cursors into storage reserved for the whole
// batch up front (every output array is bounded by the payload size), kept
// in registers rather than re-read through the packer after each byte store.
struct Writer {
  uint8_t* __restrict desc;
  uint16_t* __restrict klen;
  uint16_t* __restrict vlen;
  uint32_t* __restrict req;
  uint32_t* __restrict ent_first;
  uint32_t* __restrict desc_off;
  uint8_t* __restrict ovf;
  uint32_t* __restrict ovr;
  uint8_t* __restrict ovu;
  uint32_t* __restrict ovrule;
  size_t nb = 0, ne = 0, nd = 0;  // desc bytes, entries, descriptors
};

inline bool parse_entry(Rd r, Writer& w) {
  const uint8_t *key = nullptr, *val = nullptr;
  uint64_t kl = 0, vl = 0;
  while (r.more()) {
    const uint64_t tag = r.varint();
    if (!field_ok(tag)) return false;
    const uint32_t f = (uint32_t)(tag >> 3), wt = tag & 7;
    if ((f == 1 || f == 2) && wt == 2) {
      Rd s = r.sub();
      if (f == 1) { key = s.p; kl = s.e - s.p; }
      else { val = s.p; vl = s.e - s.p; }
    } else {
      r.skip(wt);
    }
  }
  if (!r.ok || kl > 0xFFFF || vl > 0xFFFF) return false;
  uint8_t* d = w.desc + w.nb;
  copy_small(d, key, kl);
  d[kl] = '_';
  copy_small(d + kl + 1, val, vl);
  d[kl + 1 + vl] = '_';
  w.nb += kl + vl + 2;
  w.klen[w.ne] = (uint16_t)kl;
  w.vlen[w.ne] = (uint16_t)vl;
  w.ne++;
  return true;
}

inline bool parse_descriptor(Rd r, Writer& w, uint32_t q, bool* has_limit_out) {
  bool has_limit = false;
  uint32_t rpu = 0, unit = 0;
  while (r.more()) {
    const uint64_t tag = r.varint();
    if (!field_ok(tag)) return false;
    const uint32_t f = (uint32_t)(tag >> 3), wt = tag & 7;
    if (f == 1 && wt == 2) {
      if (!parse_entry(r.sub(), w)) return false;
    } else if (f == 2 && wt == 2) {
      Rd o = r.sub();
      has_limit = true;
      while (o.more()) {
        const uint64_t t2 = o.varint();
        if (!field_ok(t2)) return false;
        const uint32_t f2 = (uint32_t)(t2 >> 3), w2 = t2 & 7;
        if (f2 == 1 && w2 == 0) rpu = (uint32_t)o.varint();
        else if (f2 == 2 && w2 == 0) unit = (uint32_t)o.varint();
        else o.skip(w2);
      }
      if (!o.ok) return false;
    } else {
      r.skip(wt);
    }
  }
  if (!r.ok) return false;
  const size_t j = w.nd++;
  w.req[j] = q;
  w.ent_first[j + 1] = (uint32_t)w.ne;
  w.desc_off[j + 1] = (uint32_t)w.nb;
  w.ovf[j] = has_limit ? 1 : 0;
  w.ovr[j] = rpu;
  w.ovu[j] = (uint8_t)(unit > 255 ? 255 : unit);
  w.ovrule[j] = 0;
  *has_limit_out = has_limit;
  return true;
}

// descriptorKey(domain, descriptor) of packed descriptor j
// (config_impl.go:300-312): domain '.' (key | key_value) joined by '.'.
void descriptor_key(rl_packer* k, const Writer& w, const uint8_t* dom, size_t dl, uint32_t j) {
  k->dkey.assign((const char*)dom, dl);
  k->dkey.push_back('.');
  const uint32_t e0 = w.ent_first[j], e1 = w.ent_first[j + 1];
  const uint8_t* p = w.desc + w.desc_off[j];
  for (uint32_t e = e0; e < e1; e++) {
    const uint32_t kl = w.klen[e], vl = w.vlen[e];
    if (e > e0) k->dkey.push_back('.');
    k->dkey.append((const char*)p, kl);
    if (vl) { k->dkey.push_back('_'); k->dkey.append((const char*)p + kl + 1, vl); }
    p += kl + vl + 2;
  }
}

uint32_t intern(rl_packer* k) {
  auto it = k->ids.find(k->dkey);
  if (it != k->ids.end()) return it->second;
  const uint32_t rule = k->first_rule + (uint32_t)k->keys.size();
  k->ids.emplace(k->dkey, rule);
  k->keys.push_back(k->dkey);
  return rule;
}

}  // namespace

extern "C" {

rl_packer* rl_packer_create(uint32_t first_override_rule) {
  rl_packer* k = new rl_packer();
  k->first_rule = first_override_rule;
  return k;
}

void rl_packer_destroy(rl_packer* k) { delete k; }

const char* rl_packer_last_error(const rl_packer* k) { return k ? k->err.c_str() : "null packer"; }

uint32_t rl_packer_rules(const rl_packer* k) { return k ? k->first_rule + (uint32_t)k->keys.size() : 0; }

const char* rl_packer_rule_key(const rl_packer* k, uint32_t rule_id) {
  if (!k || rule_id < k->first_rule || rule_id - k->first_rule >= k->keys.size()) return nullptr;
  return k->keys[rule_id - k->first_rule].c_str();
}

int rl_packer_pack(rl_packer* k, const uint8_t* msgs, const uint64_t* msg_off, uint32_t n, const int64_t* now,
                   rl_request_batch* out) {
  if (!k || !out || (n && (!msgs || !msg_off || !now))) {
    if (k) k->err = "packer: null argument";
    return RL_E_INVALID;
  }
  for (uint32_t q = 0; q < n; q++)
    if (msg_off[q + 1] < msg_off[q]) {
      k->err = "packer: message offsets must be non-decreasing";
      return RL_E_INVALID;
    }
  // every output array is bounded by the payload (an entry or descriptor costs
  // it at least 2 bytes of framing and copies no more bytes than it holds):
  // one reservation per batch, then plain stores
  const uint64_t total = n ? msg_off[n] - msg_off[0] : 0;
  const size_t cap = total / 2 + 2;
  for (auto* b : {&k->dom, &k->desc}) { b->clear(); b->reserve(total + 2); }
  for (auto* b : {&k->ovf, &k->ovu}) { b->clear(); b->reserve(cap); }
  for (auto* b : {&k->req, &k->ovr, &k->ovrule, &k->ent_first, &k->desc_off}) { b->clear(); b->reserve(cap + 1); }
  k->klen.clear(); k->klen.reserve(cap);
  k->vlen.clear(); k->vlen.reserve(cap);
  k->dom_off.clear(); k->dom_off.reserve(n + 1);
  k->hits.clear(); k->hits.reserve(n + 1);
  k->now.clear(); k->now.reserve(n + 1);
  if (n) memcpy(k->now.p, now, n * sizeof(int64_t));
  Writer w{k->desc.p, k->klen.p, k->vlen.p, k->req.p, k->ent_first.p, k->desc_off.p, k->ovf.p, k->ovr.p, k->ovu.p,
           k->ovrule.p};
  w.ent_first[0] = 0;
  w.desc_off[0] = 0;
  uint8_t* __restrict domw = k->dom.p;
  uint32_t* __restrict dom_off = k->dom_off.p;
  uint32_t* __restrict hitsw = k->hits.p;
  size_t dn = 0;
  dom_off[0] = 0;
  std::vector<uint32_t>& pend = k->pend;
  for (uint32_t q = 0; q < n; q++) {
    Rd r{msgs + msg_off[q], msgs + msg_off[q + 1]};
    const uint8_t* dom = nullptr;
    size_t dl = 0;
    uint32_t hits = 0;
    pend.clear();
    // one pass over the message; override stats keys once the domain is known
    while (r.more()) {
      const uint64_t tag = r.varint();
      if (!field_ok(tag)) { r.ok = false; break; }
      const uint32_t f = (uint32_t)(tag >> 3), wt = tag & 7;
      if (f == 2 && wt == 2) {
        bool lim = false;
        if (!parse_descriptor(r.sub(), w, q, &lim)) {
          k->err = "packer: malformed descriptor in RateLimitRequest " + std::to_string(q);
          return RL_E_INVALID;
        }
        if (lim) pend.push_back((uint32_t)(w.nd - 1));  // (its stats key needs the domain)
      } else if (f == 1 && wt == 2) {
        Rd s = r.sub();
        dom = s.p;
        dl = s.e - s.p;
      } else if (f == 3 && wt == 0) {
        hits = (uint32_t)r.varint();
      } else {
        r.skip(wt);
      }
    }
    if (!r.ok) {
      k->err = "packer: malformed RateLimitRequest " + std::to_string(q);
      return RL_E_INVALID;
    }
    for (uint32_t j : pend) {
      descriptor_key(k, w, dom, dl, j);
      w.ovrule[j] = intern(k);
    }
    copy_small(domw + dn, dom, dl);
    dn += dl;
    dom_off[q + 1] = (uint32_t)dn;
    hitsw[q] = hits;
  }
  k->desc.n = w.nb;
  k->klen.n = k->vlen.n = w.ne;
  k->req.n = k->ovr.n = k->ovrule.n = k->ovf.n = k->ovu.n = w.nd;
  k->ent_first.n = k->desc_off.n = w.nd + 1;
  k->dom.n = dn;
  k->dom_off.n = n + 1;
  k->hits.n = k->now.n = n;
  memset(out, 0, sizeof *out);
  out->n_requests = n;
  out->n_descriptors = (uint32_t)w.nd;
  out->n_entries = (uint32_t)w.ne;
  out->n_rules = rl_packer_rules(k);
  out->domain_bytes = k->dom.p;
  out->domain_off = k->dom_off.p;
  out->now = k->now.p;
  out->hits = k->hits.p;
  out->req_idx = k->req.p;
  out->entry_first = k->ent_first.p;
  out->desc_off = k->desc_off.p;
  out->desc_bytes = k->desc.p;
  out->key_len = k->klen.p;
  out->value_len = k->vlen.p;
  out->override_flags = k->ovf.p;
  out->override_rpu = k->ovr.p;
  out->override_unit = k->ovu.p;
  out->override_rule = k->ovrule.p;
  k->err.clear();
  return RL_OK;
}

// rl_request_batch -> the one-buffer layout of rl_request_batch_packed. Two
// passes: the first only reads and checks (so a refused batch leaves buf as
// it was), the second writes the sections and the tile index.
int rl_request_batch_pack(const rl_request_batch* in, uint8_t* buf, uint64_t buf_cap, rl_request_batch_packed* out) {
  if (!in || !out) return RL_E_INVALID;
  const uint32_t nq = in->n_requests, n = in->n_descriptors, ne = in->n_entries;
  if (!in->domain_off || !in->entry_first || !in->desc_off || (nq && (!in->now || !in->hits)) ||
      (n && (!in->req_idx || !nq)) || (ne && (!in->key_len || !in->value_len)))
    return RL_E_INVALID;
  if (in->override_flags && (!in->override_rpu || !in->override_unit || !in->override_rule)) return RL_E_INVALID;
  if (in->domain_off[0] || in->entry_first[0] || in->desc_off[0] || in->entry_first[n] != ne) return RL_E_INVALID;
  for (uint32_t q = 0; q < nq; q++) {
    if (in->domain_off[q + 1] < in->domain_off[q] || in->domain_off[q + 1] - in->domain_off[q] > 65535u)
      return RL_E_INVALID;
    if (in->now[q] < 0 || in->now[q] > (int64_t)0xFFFFFFFFll) return RL_E_INVALID;
  }
  uint32_t nov = 0;
  for (uint32_t d = 0, run = 0; d < n; d++) {
    const uint32_t q = in->req_idx[d];
    if (q >= nq || (d && q < in->req_idx[d - 1])) return RL_E_INVALID;
    run = (d && q == in->req_idx[d - 1]) ? run + 1 : 1;
    if (run > 65535u) return RL_E_INVALID;
    const uint32_t e0 = in->entry_first[d], e1 = in->entry_first[d + 1];
    if (e1 < e0 || e1 > ne || e1 - e0 > 65535u || in->desc_off[d + 1] < in->desc_off[d]) return RL_E_INVALID;
    uint64_t bytes = 0;
    for (uint32_t e = e0; e < e1; e++) bytes += (uint64_t)in->key_len[e] + in->value_len[e] + 2u;
    if (bytes != (uint64_t)(in->desc_off[d + 1] - in->desc_off[d])) return RL_E_INVALID;
    if (in->override_flags && (in->override_flags[d] & 1u)) nov++;
  }
  const uint32_t dom_total = in->domain_off[nq], ent_total = in->desc_off[n];
  if ((dom_total && !in->domain_bytes) || (ent_total && !in->desc_bytes)) return RL_E_INVALID;
  const uint32_t tiles = (nq + RL_REQUESTS_TILE - 1) / RL_REQUESTS_TILE;
  uint64_t need = 0;
  auto section = [&need](uint64_t bytes) {
    const uint64_t o = need;
    need += (bytes + 3) & ~3ull;
    return o;
  };
  rl_request_batch_packed p;
  memset(&p, 0, sizeof p);
  p.n_requests = nq;
  p.n_descriptors = n;
  p.n_entries = ne;
  p.n_rules = in->n_rules;
  p.n_overrides = nov;
  p.index = section(16ull * (tiles + 1));
  p.req = section(4ull * nq);
  p.now = section(4ull * nq);
  p.hits = section(4ull * nq);
  p.desc = section(2ull * n);
  p.key_len = section(2ull * ne);
  p.value_len = section(2ull * ne);
  p.overrides = section(sizeof(rl_request_override) * (uint64_t)nov);
  p.domain_bytes = section(dom_total);
  p.entry_bytes = section(ent_total);
  if (!buf || buf_cap < need) {
    out->buf_bytes = need;
    return RL_E_CAPACITY;
  }
  p.buf = buf;
  p.buf_bytes = need;
  // (the sections' padding to 4 bytes is written too: the buffer is a function of the batch)
  auto put = [buf](uint64_t off, const void* src, uint64_t bytes) {
    if (bytes) memcpy(buf + off, src, bytes);
    memset(buf + off + bytes, 0, ((bytes + 3) & ~3ull) - bytes);
  };
  uint32_t* index = reinterpret_cast<uint32_t*>(buf + p.index);
  uint32_t* req = reinterpret_cast<uint32_t*>(buf + p.req);
  uint32_t* now = reinterpret_cast<uint32_t*>(buf + p.now);
  uint16_t* desc = reinterpret_cast<uint16_t*>(buf + p.desc);
  rl_request_override* ov = reinterpret_cast<rl_request_override*>(buf + p.overrides);
  uint32_t d = 0;
  for (uint32_t q = 0; q < nq; q++) {
    if (q % RL_REQUESTS_TILE == 0) {
      uint32_t* ix = index + 4ull * (q / RL_REQUESTS_TILE);
      ix[0] = d;
      ix[1] = in->entry_first[d];
      ix[2] = in->domain_off[q];
      ix[3] = in->desc_off[d];
    }
    const uint32_t d0 = d;
    while (d < n && in->req_idx[d] == q) d++;
    req[q] = (d - d0) | (in->domain_off[q + 1] - in->domain_off[q]) << 16;
    now[q] = (uint32_t)in->now[q];
  }
  uint32_t* tot = index + 4ull * tiles;
  tot[0] = n;
  tot[1] = ne;
  tot[2] = dom_total;
  tot[3] = ent_total;
  put(p.hits, in->hits, 4ull * nq);
  for (uint32_t i = 0, k = 0; i < n; i++) {
    desc[i] = (uint16_t)(in->entry_first[i + 1] - in->entry_first[i]);
    if (in->override_flags && (in->override_flags[i] & 1u)) {
      rl_request_override& o = ov[k++];
      o.descriptor = i;
      o.requests_per_unit = in->override_rpu[i];
      o.rule_id = in->override_rule[i];
      o.unit = in->override_unit[i];
      o.reserved[0] = o.reserved[1] = o.reserved[2] = 0;
    }
  }
  if (n & 1u) desc[n] = 0;
  put(p.key_len, in->key_len, 2ull * ne);
  put(p.value_len, in->value_len, 2ull * ne);
  put(p.domain_bytes, in->domain_bytes, dom_total);
  put(p.entry_bytes, in->desc_bytes, ent_total);
  *out = p;
  return RL_OK;
}


// ---- serialized RateLimitResponse payloads: the host twin of rl_resp.hip -----

uint64_t rl_response_bound(uint32_t n_requests, uint32_t n_descriptors, const rl_response_format* fmt) {
  rlresp::Format f;
  if (!rlresp::format_from(fmt, &f)) return 0;
  return rlresp::bound(n_requests, n_descriptors, f);
}

namespace {
struct HostSink {
  uint8_t* p;
  void put(uint8_t b) { *p++ = b; }
};
}  // namespace

// Two passes, like the device: the sizes into resp_off, then the bytes.
int rl_response_serialize(uint32_t nq, const uint32_t* desc_first, const uint8_t* req_status,
                          const rl_request_result* res, const rl_request_verdict* v, const rl_response_format* fmt,
                          uint8_t* bytes, uint64_t bytes_cap, uint32_t* resp_off, uint64_t* bytes_needed) {
  rlresp::Format f;
  if (!desc_first || !v || !resp_off || !rlresp::format_from(fmt, &f)) return RL_E_INVALID;
  if (desc_first[0]) return RL_E_INVALID;
  const uint32_t n = desc_first[nq];
  if (nq && !v->overall_code) return RL_E_INVALID;
  if (nq && f.headers && (!v->min_descriptor || !v->header_limit || !v->header_remaining || !v->header_reset_s))
    return RL_E_INVALID;
  if (n && (!res || !res->code || !res->limit_remaining || !res->reset_s || !res->match || !res->requests_per_unit ||
            !res->unit))
    return RL_E_INVALID;
  auto status = [res](uint32_t d) {
    return rlresp::Status{res->code[d], res->match[d], res->requests_per_unit[d], res->unit[d],
                          res->limit_remaining[d], res->reset_s[d]};
  };
  auto hdr = [&](uint32_t q) -> uint32_t {
    if (!f.headers || desc_first[q + 1] == desc_first[q]) return 0;
    return rlresp::headers_size(f, v->min_descriptor[q], v->header_limit[q], v->header_remaining[q],
                                v->header_reset_s[q]);
  };
  uint64_t total = 0;
  for (uint32_t q = 0; q < nq; q++) {
    if (desc_first[q + 1] < desc_first[q]) return RL_E_INVALID;
    if (req_status && req_status[q] != RL_WIRE_OK && desc_first[q + 1] != desc_first[q]) return RL_E_INVALID;
  }
  for (uint32_t q = 0; q < nq; q++) {
    resp_off[q] = (uint32_t)total;
    if (req_status && req_status[q] != RL_WIRE_OK) continue;
    total += rlresp::head_size(v->overall_code[q]) + hdr(q);
    for (uint32_t d = desc_first[q]; d < desc_first[q + 1]; d++) total += rlresp::status_size(status(d));
    if (total >> 32) return RL_E_CAPACITY;  // (resp_off is 32-bit)
  }
  resp_off[nq] = (uint32_t)total;
  if (bytes_needed) *bytes_needed = total;
  if (total > bytes_cap || (total && !bytes)) return RL_E_CAPACITY;
  HostSink s{bytes};
  for (uint32_t q = 0; q < nq; q++) {
    if (req_status && req_status[q] != RL_WIRE_OK) continue;
    rlresp::emit_head(v->overall_code[q], s);
    for (uint32_t d = desc_first[q]; d < desc_first[q + 1]; d++) rlresp::emit_status(status(d), s);
    if (hdr(q))
      rlresp::emit_headers(f, v->min_descriptor[q], v->header_limit[q], v->header_remaining[q], v->header_reset_s[q], s);
  }
  return RL_OK;
}

}  // extern "C"
