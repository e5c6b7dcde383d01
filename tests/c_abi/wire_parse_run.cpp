// wire_parse_run.cpp — the device parser's per-message walk
// (ratelimit_amd/csrc/rl_wire_parse.h) on the CPU (test program, its own
// main; built plain and with -fsanitize=address,undefined by
// tests/test_wire_cpu.py). Input file: uint32 count, then per message uint32
// length and its bytes. Per message the count walk, then for an OK message the
// emit walk into arrays sized by the counts, as k_wire_count and k_wire_emit
// do. Each message is walked in a heap block of exactly its size, so a read
// past its end is an AddressSanitizer finding. Output per message:
//   M <index> <status> <fnv1a-64 of the emitted arrays, 0 unless OK>
// The hashed bytes, little endian: u32 descriptors, entries, hits, domain
// bytes, entry bytes; u32 req[nd]; u32 ent_first[nd + 1]; u32 desc_off[nd + 1];
// u16 klen[ne]; u16 vlen[ne]; the domain bytes; the entry bytes.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rl_wire_parse.h"

namespace {

struct HostSrc {
  const uint8_t* p;
  uint8_t operator[](uint32_t i) const { return p[i]; }
};

// The emit walk's sink on the host: every store inside the counted share.
struct HostEmit {
  std::vector<uint32_t> req, ent_first, desc_off;
  std::vector<uint16_t> klen, vlen;
  std::vector<uint8_t> ent;
  uint32_t d = 0, e = 0, bo = 0, de = 0, db = 0;
  bool bad = false;
  HostEmit(uint32_t nd, uint32_t ne, uint32_t eb)
      : req(nd), ent_first(nd + 1), desc_off(nd + 1), klen(ne), vlen(ne), ent(eb) {}
  void entry(const HostSrc& b, uint32_t kp, uint32_t kn, uint32_t vp, uint32_t vn) {
    const uint32_t len = kn + vn + 2u;
    if (bad || e >= klen.size() || len > ent.size() - bo) {
      bad = true;
      return;
    }
    uint8_t* dst = ent.data() + bo;
    for (uint32_t i = 0; i < kn; i++) dst[i] = b[kp + i];
    dst[kn] = '_';
    dst += kn + 1u;
    for (uint32_t i = 0; i < vn; i++) dst[i] = b[vp + i];
    dst[vn] = '_';
    klen[e] = (uint16_t)kn;
    vlen[e] = (uint16_t)vn;
    e++;
    bo += len;
  }
  void descriptor(uint32_t) {
    if (bad || d >= req.size()) {
      bad = true;
      return;
    }
    req[d] = 0;
    ent_first[d] = de;
    desc_off[d] = db;
    d++;
    de = e;
    db = bo;
  }
};

struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void bytes(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  }
  void u32(uint32_t v) { bytes(&v, 4); }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t len = 0;
    if (fread(&len, 4, 1, f) != 1) return 2;
    uint8_t* msg = new uint8_t[len];  // (exactly its size)
    if (len && fread(msg, 1, len, f) != len) return 2;
    const HostSrc src{msg};
    rlwire::CountSink cs;
    const rlwire::Message m = rlwire::walk_message(src, 0u, len, cs);
    uint64_t hash = 0;
    if (m.status == rlwire::ST_OK) {
      HostEmit em(m.n_desc, cs.n_ent, cs.ent_bytes);
      const rlwire::Message m2 = rlwire::walk_message(src, 0u, len, em);
      if (em.bad || m2.status != m.status || m2.n_desc != m.n_desc || em.d != m.n_desc || em.e != cs.n_ent ||
          em.bo != cs.ent_bytes || m2.dom_len != m.dom_len || m2.dom_pos != m.dom_pos || m2.hits != m.hits) {
        fprintf(stderr, "message %u: the emit walk left the count walk's share\n", i);
        return 3;
      }
      em.ent_first[em.d] = em.e;
      em.desc_off[em.d] = em.bo;
      Fnv h;
      h.u32(m.n_desc);
      h.u32(cs.n_ent);
      h.u32(m.hits);
      h.u32(m.dom_len);
      h.u32(cs.ent_bytes);
      h.bytes(em.req.data(), em.req.size() * 4);
      h.bytes(em.ent_first.data(), em.ent_first.size() * 4);
      h.bytes(em.desc_off.data(), em.desc_off.size() * 4);
      h.bytes(em.klen.data(), em.klen.size() * 2);
      h.bytes(em.vlen.data(), em.vlen.size() * 2);
      h.bytes(msg + m.dom_pos, m.dom_len);
      h.bytes(em.ent.data(), em.ent.size());
      hash = h.h;
    }
    printf("M %u %u %016llx\n", i, m.status, (unsigned long long)hash);
    delete[] msg;
  }
  fclose(f);
  return 0;
}
