// rl_wire_parse.h — the walk over one serialized
// envoy.service.ratelimit.v3.RateLimitRequest, shared by the device parser
// (rl_wire.hip: k_wire_count, k_wire_emit) and a host driver
// (tests/c_abi/wire_parse_run.cpp). Plain C++; RLW_HD is __host__ __device__
// under hipcc and empty otherwise.
//
// The host packer (rl_pack.cpp) is the authority: a message is malformed
// exactly where rl_packer_pack on it alone returns RL_E_INVALID, and every
// accepted message gives the packer's arrays. Every read is bounded by the
// message's own end [p, e). B is a byte source with operator[](uint32_t).
//
// The walk reports to a sink S:
//   s.entry(b, key_pos, key_len, value_pos, value_len)   one Entry, in order
//   s.descriptor(entries)                               one RateLimitDescriptor ended
//   s.limit(b, ordinal, rpu, unit, desc_pos, desc_end)  (optional member) a descriptor with `limit`
// A sink bounds its own stores; the walk never stores.
//
// Overrides: walk_message<B, S, true> (the default) defers every message that
// carries a descriptor with `limit`, as before. walk_message<B, S, false>
// parses the override as rl_pack.cpp's parse_descriptor does (the last written
// requests_per_unit and unit win across repeated `limit` fields, rpu truncated
// to 32 bits, unit clamped to 255) and reports it to the sink's limit() member,
// if it has one, when the descriptor ends: its ordinal in the message and the
// descriptor's own bytes [desc_pos, desc_end), from which descriptor_key()
// streams descriptorKey(domain, descriptor) once the message's domain is known.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RLW_HD __host__ __device__ __forceinline__
#else
#define RLW_HD inline
#endif

namespace rlwire {

// == enum rl_wire_status (include/ratelimit_hip.h)
constexpr uint32_t ST_OK = 0, ST_DEFERRED = 1, ST_MALFORMED = 2;
constexpr uint32_t ITEM_MAX = 65535u;  // the packed layout's per-item limits

template <class B>
struct Rd {
  B b;
  uint32_t p, e;
  bool ok;
  RLW_HD bool more() const { return ok && p < e; }
  RLW_HD uint64_t varint() {
    uint64_t v = 0;
    for (uint32_t s = 0; s < 64; s += 7) {  // (10 bytes at the most)
      if (p >= e) { ok = false; return 0; }
      const uint8_t c = b[p++];
      v |= (uint64_t)(c & 0x7Fu) << s;
      if (!(c & 0x80u)) return v;
    }
    ok = false;
    return 0;
  }
  // a length-delimited field's bytes
  RLW_HD Rd sub() {
    const uint64_t n = varint();
    if (!ok || n > (uint64_t)(e - p)) { ok = false; return Rd{b, p, p, true}; }
    Rd r{b, p, p + (uint32_t)n, true};
    p += (uint32_t)n;
    return r;
  }
  RLW_HD void skip(uint32_t wt) {
    if (wt == 0) (void)varint();
    else if (wt == 1) { if (e - p < 8u) ok = false; else p += 8u; }
    else if (wt == 2) (void)sub();
    else if (wt == 5) { if (e - p < 4u) ok = false; else p += 4u; }
    else ok = false;  // groups (3, 4) and the undefined types 6, 7
  }
};

RLW_HD bool field_ok(uint64_t tag) { return (tag >> 3) != 0 && (tag >> 3) <= 0x1FFFFFFFull; }

// Entry: 1 key, 2 value; the last of each wins. False: malformed.
template <class B, class S>
RLW_HD bool walk_entry(Rd<B> r, S& s) {
  uint32_t kp = 0, kl = 0, vp = 0, vl = 0;
  while (r.more()) {
    const uint64_t tag = r.varint();
    if (!field_ok(tag)) return false;
    const uint32_t f = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7u);
    if ((f == 1 || f == 2) && wt == 2) {
      const Rd<B> x = r.sub();
      if (f == 1) { kp = x.p; kl = x.e - x.p; }
      else { vp = x.p; vl = x.e - x.p; }
    } else {
      r.skip(wt);
    }
  }
  if (!r.ok || kl > ITEM_MAX || vl > ITEM_MAX) return false;
  s.entry(r.b, kp, kl, vp, vl);
  return true;
}

// s.limit(...) where S has such a member; nothing otherwise.
template <class B, class S>
RLW_HD auto report_limit(S& s, const B& b, uint32_t ord, uint32_t rpu, uint32_t unit, uint32_t p, uint32_t e, int)
    -> decltype(s.limit(b, ord, rpu, unit, p, e), void()) {
  s.limit(b, ord, rpu, unit, p, e);
}
template <class B, class S>
RLW_HD void report_limit(S&, const B&, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, long) {}

// RateLimitDescriptor: 1 entries, 2 limit (RateLimitOverride: 1, 2 varints).
// False: malformed. *defer is set for more than ITEM_MAX entries and, with
// DEFER_OV, for an override; without it the override is reported to the sink.
template <bool DEFER_OV, class B, class S>
RLW_HD bool walk_descriptor(Rd<B> r, S& s, bool* defer, uint32_t ord) {
  uint32_t ne = 0;
  const uint32_t p0 = r.p;
  bool has_limit = false;
  uint32_t rpu = 0, unit = 0;
  while (r.more()) {
    const uint64_t tag = r.varint();
    if (!field_ok(tag)) return false;
    const uint32_t f = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7u);
    if (f == 1 && wt == 2) {
      const Rd<B> x = r.sub();
      if (!r.ok || !walk_entry(x, s)) return false;
      ne++;
    } else if (f == 2 && wt == 2) {
      Rd<B> o = r.sub();
      if (!r.ok) return false;
      if (DEFER_OV) *defer = true;
      else has_limit = true;
      while (o.more()) {
        const uint64_t t2 = o.varint();
        if (!field_ok(t2)) return false;
        const uint32_t f2 = (uint32_t)(t2 >> 3), w2 = (uint32_t)(t2 & 7u);
        if ((f2 == 1 || f2 == 2) && w2 == 0) {
          const uint32_t v = (uint32_t)o.varint();
          if (!DEFER_OV) {
            if (f2 == 1) rpu = v;
            else unit = v;
          }
        } else {
          o.skip(w2);
        }
      }
      if (!o.ok) return false;
    } else {
      r.skip(wt);
    }
  }
  if (!r.ok) return false;
  if (ne > ITEM_MAX) *defer = true;
  s.descriptor(ne);
  if (!DEFER_OV && has_limit) report_limit(s, r.b, ord, rpu, unit > 255u ? 255u : unit, p0, r.e, 0);
  return true;
}

struct Message {
  uint32_t status;            // ST_*
  uint32_t n_desc;
  uint32_t dom_pos, dom_len;  // the last domain field (positions index the byte source)
  uint32_t hits;              // the last hits_addend, truncated to 32 bits
};

// RateLimitRequest at [p, e): 1 domain, 2 descriptors, 3 hits_addend.
template <class B, class S, bool DEFER_OV = true>
RLW_HD Message walk_message(B b, uint32_t p, uint32_t e, S& s) {
  Rd<B> r{b, p, e, true};
  Message m{ST_OK, 0, p, 0, 0};
  bool defer = false;
  while (r.more()) {
    const uint64_t tag = r.varint();
    if (!field_ok(tag)) { r.ok = false; break; }
    const uint32_t f = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7u);
    if (f == 2 && wt == 2) {
      const Rd<B> x = r.sub();
      if (!r.ok || !walk_descriptor<DEFER_OV>(x, s, &defer, m.n_desc)) { r.ok = false; break; }
      m.n_desc++;
    } else if (f == 1 && wt == 2) {
      const Rd<B> x = r.sub();
      m.dom_pos = x.p;
      m.dom_len = x.e - x.p;
    } else if (f == 3 && wt == 0) {
      m.hits = (uint32_t)r.varint();
    } else {
      r.skip(wt);
    }
  }
  if (!r.ok) m.status = ST_MALFORMED;
  else if (defer || m.n_desc > ITEM_MAX || m.dom_len > ITEM_MAX) m.status = ST_DEFERRED;
  return m;
}

// The count walk's sink: entries and entry bytes Σ(key_len + value_len + 2).
struct CountSink {
  uint32_t n_ent = 0, ent_bytes = 0;
  template <class B>
  RLW_HD void entry(const B&, uint32_t, uint32_t kl, uint32_t, uint32_t vl) {
    n_ent++;
    ent_bytes += kl + vl + 2u;
  }
  RLW_HD void descriptor(uint32_t) {}
};

// descriptorKey(domain, descriptor) (config_impl.go:300-312) of the descriptor
// whose bytes are [p, e) of a message the walk accepted, streamed to f:
//   f.bytes(b, pos, len)   len bytes of the source from pos
//   f.sep(c)               one separator byte
// domain '.' then per entry, joined by '.': key, and '_' value when the value
// is not empty (so ("a_b", "") and ("a", "b") are one key). The last key and
// value of an entry win, as in walk_entry. Nothing is staged: a functor that
// only adds lengths costs no byte read.
template <class B, class F>
RLW_HD void descriptor_key(const B& b, uint32_t dom_pos, uint32_t dom_len, uint32_t p, uint32_t e, F& f) {
  f.bytes(b, dom_pos, dom_len);
  f.sep('.');
  Rd<B> r{b, p, e, true};
  bool first = true;
  while (r.more()) {
    const uint64_t tag = r.varint();
    const uint32_t fn = (uint32_t)(tag >> 3), wt = (uint32_t)(tag & 7u);
    if (fn == 1 && wt == 2) {
      Rd<B> x = r.sub();
      if (!r.ok) return;
      uint32_t kp = 0, kl = 0, vp = 0, vl = 0;
      while (x.more()) {
        const uint64_t t2 = x.varint();
        const uint32_t f2 = (uint32_t)(t2 >> 3), w2 = (uint32_t)(t2 & 7u);
        if ((f2 == 1 || f2 == 2) && w2 == 2) {
          const Rd<B> y = x.sub();
          if (f2 == 1) { kp = y.p; kl = y.e - y.p; }
          else { vp = y.p; vl = y.e - y.p; }
        } else {
          x.skip(w2);
        }
      }
      if (!x.ok) return;
      if (!first) f.sep('.');
      first = false;
      f.bytes(b, kp, kl);
      if (vl) {
        f.sep('_');
        f.bytes(b, vp, vl);
      }
    } else {
      r.skip(wt);
    }
  }
}

// descriptor_key's length alone.
struct KeyLen {
  uint64_t n = 0;
  template <class B>
  RLW_HD void bytes(const B&, uint32_t, uint32_t len) { n += len; }
  RLW_HD void sep(uint8_t) { n++; }
};

}  // namespace rlwire
