// wire_override_run.cpp — the device parser's walk with overrides reported
// (ratelimit_amd/csrc/rl_wire_parse.h, walk_message<B, S, false>) on the CPU
// (test program, its own main; built plain and with
// -fsanitize=address,undefined by tests/test_wire_override_cpu.py). Input file:
// uint32 count, then per message uint32 length and its bytes. Each message is
// walked in a heap block of exactly its size, so a read past its end is an
// AddressSanitizer finding. Per message the walk that defers overrides (the
// not-enabled path), then the walk that reports them to a sink with a limit()
// member, as k_wire_count does on an enabled ctx; for every reported override
// of a well-formed message its descriptorKey is streamed by descriptor_key()
// once the domain is known. Output per message:
//   M <index> <status, overrides deferred> <status, overrides reported> <descriptors> <overrides>
//   D <ordinal> <requests_per_unit> <unit> <key length> <the key's bytes in hex, "-" when empty>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "rl_wire_parse.h"

namespace {

struct HostSrc {
  const uint8_t* p;
  uint8_t operator[](uint32_t i) const { return p[i]; }
};

struct Override {
  uint32_t ord, rpu, unit, p, e;
};

// The count walk's sink with the optional member: every override recorded.
struct OvSink : rlwire::CountSink {
  std::vector<Override> ov;
  void limit(const HostSrc&, uint32_t ord, uint32_t rpu, uint32_t unit, uint32_t p, uint32_t e) {
    ov.push_back(Override{ord, rpu, unit, p, e});
  }
};

// descriptor_key's bytes, collected.
struct KeyBytes {
  std::string s;
  void bytes(const HostSrc& b, uint32_t pos, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) s.push_back((char)b[pos + i]);
  }
  void sep(uint8_t c) { s.push_back((char)c); }
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
    rlwire::CountSink plain;
    const rlwire::Message m0 = rlwire::walk_message(src, 0u, len, plain);
    OvSink s;
    const rlwire::Message m = rlwire::walk_message<HostSrc, OvSink, false>(src, 0u, len, s);
    // a sink without the member on the reporting walk: nothing reported, nothing deferred for an override
    rlwire::CountSink mute;
    const rlwire::Message m1 = rlwire::walk_message<HostSrc, rlwire::CountSink, false>(src, 0u, len, mute);
    if (m1.status != m.status || mute.n_ent != s.n_ent || mute.ent_bytes != s.ent_bytes ||
        (m0.status == rlwire::ST_MALFORMED) != (m.status == rlwire::ST_MALFORMED) ||
        (m.status != rlwire::ST_MALFORMED && (plain.n_ent != s.n_ent || m0.n_desc != m.n_desc ||
                                              m0.dom_pos != m.dom_pos || m0.dom_len != m.dom_len))) {
      fprintf(stderr, "message %u: the walks disagree\n", i);
      return 3;
    }
    const bool good = m.status != rlwire::ST_MALFORMED;
    printf("M %u %u %u %u %zu\n", i, m0.status, m.status, good ? m.n_desc : 0u, good ? s.ov.size() : (size_t)0);
    if (good) {
      for (const Override& o : s.ov) {
        rlwire::KeyLen L;
        rlwire::descriptor_key(src, m.dom_pos, m.dom_len, o.p, o.e, L);
        KeyBytes k;
        rlwire::descriptor_key(src, m.dom_pos, m.dom_len, o.p, o.e, k);
        if (L.n != k.s.size()) {
          fprintf(stderr, "message %u: descriptor_key's length and bytes disagree\n", i);
          return 3;
        }
        printf("D %u %u %u %zu ", o.ord, o.rpu, o.unit, k.s.size());
        if (k.s.empty()) printf("-");
        for (unsigned char c : k.s) printf("%02x", c);
        printf("\n");
      }
    }
    delete[] msg;
  }
  fclose(f);
  return 0;
}
