// rl_request_layout.h — the arithmetic of the request path's host layer
// (rl_requests.hip): how one device buffer is carved into the arrays of a
// batch, and the bounds checks of a one-buffer batch's sections and tile
// index. The sizes the kernels' own headers define (match_scan_bytes,
// verdict_layout(nq).bytes, resp_layout(...).total) come in as numbers. Plain
// C++, also built by tests/c_abi/request_layout_run.cpp. (static: no symbol
// of these leaves the library.)
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rlreq {

// One device buffer cut into 256-byte aligned pieces. A piece of no bytes
// still takes 256: every array has an address of its own.
struct Carve {
  size_t need = 0;  // the buffer's size so far
  size_t piece(size_t bytes) {
    const size_t o = need;
    need += ((bytes ? bytes : 1) + 255) & ~(size_t)255;
    return o;
  }
};

// The match stage's arrays over n descriptors, which every buffer that feeds
// launch_match holds: MatchBuf (v .. cnt), ReqOutDev (code .. ounit), the
// scan's scratch and, when asked for, the verdict block. (The members stand in
// carve order: braces evaluate left to right.)
struct MatchPieces {
  size_t v, kind, rpu, rule, cnt, code, rem, reset, match, orule, orpu, ounit, tmp, verdict;
};
static inline MatchPieces match_pieces(Carve& c, size_t n, size_t scan, bool want_verdict, size_t verdict_bytes) {
  return {c.piece(n * 16), c.piece(n * 4), c.piece(n * 4), c.piece(n * 4), c.piece(16), c.piece(n), c.piece(n * 4),
          c.piece(n * 4), c.piece(n), c.piece(n * 4), c.piece(n * 4), c.piece(n), c.piece(scan),
          want_verdict ? c.piece(verdict_bytes) : 0};
}

// A section of a one-buffer batch: 4-byte aligned and inside the B bytes of buf.
static inline bool in_buf(uint64_t B, uint64_t off, uint64_t bytes) {
  return off % 4 == 0 && off <= B && bytes <= B - off;
}

// Tiles of `tile` requests that nq requests take.
static inline uint32_t tiles(uint32_t nq, uint32_t tile) { return (nq + tile - 1) / tile; }

// A tile index (T + 1 entries of four words): its first entry zero and its
// last the batch's n descriptors (and ne entries: the packed request batch).
static inline bool index_ends_ok(const uint32_t* ix, uint32_t T, uint32_t n) {
  return !(ix[0] | ix[1] | ix[2] | ix[3]) && ix[4ull * T] == n;
}
static inline bool index_ends_ok(const uint32_t* ix, uint32_t T, uint32_t n, uint32_t ne) {
  return index_ends_ok(ix, T, n) && ix[4ull * T + 1] == ne;
}

}  // namespace rlreq
