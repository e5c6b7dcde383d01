// Host driver of rl_request_layout.h (tests/test_request_layout_cpu.py): one
// query per input line, one answer line each. The four buffers are carved here
// as rl_requests.hip carves them: the same piece lists over Carve and
// match_pieces; the sizes the kernels' headers define come in as numbers.
//   sync n nq ne dom desc ovr scan verdict vbytes      -> total name=offset ...
//   packed n nq ovr scan verdict vbytes
//   wiremid n nq ne dom ent ovr scan verdict vbytes resp rbytes
//   wbuf nq T ovr
//   in_buf B off bytes                                  -> 0 | 1
//   ends T n ne|- w...  (the index's 4 (T + 1) words)   -> 0 | 1
//   tiles nq tile                                       -> tiles
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rl_request_layout.h"

using rlreq::Carve;

static void put(const char* name, size_t off) { printf(" %s=%zu", name, off); }

static void put_match(const rlreq::MatchPieces& p, bool verdict) {
  const char* names[] = {"v", "kind", "rpu", "rule", "cnt", "code", "rem", "reset", "match", "orule", "orpu", "ounit", "tmp"};
  const size_t offs[] = {p.v, p.kind, p.rpu, p.rule, p.cnt, p.code, p.rem, p.reset, p.match, p.orule, p.orpu, p.ounit, p.tmp};
  for (int i = 0; i < 13; i++) put(names[i], offs[i]);
  if (verdict) put("verdict", p.verdict);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    Carve cv;
    if (op == "sync") {
      size_t n, nq, ne, dom, desc, ovr, scan, verdict, vbytes;
      in >> n >> nq >> ne >> dom >> desc >> ovr >> scan >> verdict >> vbytes;
      const size_t o[] = {cv.piece(dom), cv.piece((nq + 1) * 4), cv.piece(nq * 4), cv.piece(n * 4), cv.piece((n + 1) * 4),
                          cv.piece((n + 1) * 4), cv.piece(desc), cv.piece(ne * 2), cv.piece(ne * 2), cv.piece(ovr ? n : 0),
                          cv.piece(ovr ? n * 4 : 0), cv.piece(ovr ? n : 0), cv.piece(ovr ? n * 4 : 0)};
      const rlreq::MatchPieces mp = rlreq::match_pieces(cv, n, scan, verdict != 0, vbytes);
      printf("%zu", cv.need);
      const char* names[] = {"dom", "domoff", "hits", "req", "ent", "doff", "desc", "kl", "vl", "ovf", "ovr", "ovu", "ovrule"};
      for (int i = 0; i < 13; i++) put(names[i], o[i]);
      put_match(mp, verdict != 0);
    } else if (op == "packed") {
      size_t n, nq, ovr, scan, verdict, vbytes;
      in >> n >> nq >> ovr >> scan >> verdict >> vbytes;
      const size_t o[] = {cv.piece((nq + 1) * 4), cv.piece(n * 4), cv.piece((n + 1) * 4), cv.piece((n + 1) * 4),
                          cv.piece(ovr ? n * 10 : 0)};
      const rlreq::MatchPieces mp = rlreq::match_pieces(cv, n, scan, verdict != 0, vbytes);
      printf("%zu", cv.need);
      const char* names[] = {"domoff", "req", "ent", "doff", "ov"};
      for (int i = 0; i < 5; i++) put(names[i], o[i]);
      put_match(mp, verdict != 0);
    } else if (op == "wiremid") {
      size_t n, nq, ne, dom, ent, ovr, scan, verdict, vbytes, resp, rbytes;
      in >> n >> nq >> ne >> dom >> ent >> ovr >> scan >> verdict >> vbytes >> resp >> rbytes;
      const size_t o[] = {cv.piece((nq + 1) * 4), cv.piece(n * 4), cv.piece((n + 1) * 4), cv.piece((n + 1) * 4),
                          cv.piece(nq * 4), cv.piece(ne * 2), cv.piece(ne * 2), cv.piece(dom), cv.piece(ent)};
      const rlreq::MatchPieces mp = rlreq::match_pieces(cv, n, scan, verdict != 0, vbytes);
      const size_t o_ov = ovr ? cv.piece(n * 10) : 0, o_resp = resp ? cv.piece(rbytes) : 0;
      printf("%zu", cv.need);
      const char* names[] = {"domoff", "req", "ent", "doff", "hits", "klen", "vlen", "dom", "desc"};
      for (int i = 0; i < 9; i++) put(names[i], o[i]);
      put_match(mp, verdict != 0);
      if (ovr) put("ov", o_ov);
      if (resp) put("resp", o_resp);
    } else if (op == "wbuf") {
      size_t nq, T, ovr;
      in >> nq >> T >> ovr;
      const size_t o[] = {cv.piece(nq * 16), cv.piece(T * 16), cv.piece((T + 1) * 16), cv.piece(32), cv.piece(nq),
                          cv.piece((nq + 1) * 4)};
      const size_t o_miss = ovr ? cv.piece(nq * 4) : 0;
      printf("%zu", cv.need);
      const char* names[] = {"reqw", "tsum", "index", "cnt", "status", "first"};
      for (int i = 0; i < 6; i++) put(names[i], o[i]);
      if (ovr) put("miss", o_miss);
    } else if (op == "in_buf") {
      uint64_t B, off, bytes;
      in >> B >> off >> bytes;
      printf("%d", rlreq::in_buf(B, off, bytes) ? 1 : 0);
    } else if (op == "ends") {
      uint32_t T, n;
      std::string ne;
      in >> T >> n >> ne;
      std::vector<uint32_t> ix(4 * ((size_t)T + 1));
      for (uint32_t& w : ix) in >> w;
      const bool ok = ne == "-" ? rlreq::index_ends_ok(ix.data(), T, n)
                                : rlreq::index_ends_ok(ix.data(), T, n, (uint32_t)std::stoul(ne));
      printf("%d", ok ? 1 : 0);
    } else if (op == "tiles") {
      uint32_t nq, tile;
      in >> nq >> tile;
      printf("%" PRIu32, rlreq::tiles(nq, tile));
    } else {
      return 2;
    }
    printf("\n");
  }
  return 0;
}
