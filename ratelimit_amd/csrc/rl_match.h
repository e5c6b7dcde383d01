// rl_match.h — the config trie on the device and the kernels of the request
// path (rl_match.hip): GetLimit per descriptor, compaction of the matched
// descriptors into the DoLimit batch, and the service's status mapping.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_resp_emit.h"

namespace rl {

// One config node on the device (rl_config_node plus its child count).
struct CfgNode {
  int32_t parent;
  uint32_t key_off, key_len;
  uint32_t rpu, rule;
  uint32_t n_children;
  uint8_t unit, has_limit, unlimited, shadow;
  uint32_t pad;
};

// The loaded config: nodes, their key bytes and an open-addressing index of
// (parent, key) -> node. Index entries: tag (high hash bits) | (node + 1) << 32;
// 0 = empty. Collision-exact: a tag match is confirmed with the key bytes.
struct CfgDev {
  const CfgNode* nodes;
  const uint8_t* keys;
  const unsigned long long* index;
  uint32_t mask;      // index size - 1
  uint32_t n_nodes;
  const uint8_t* prefix;
  uint32_t prefix_len;
  // the whole config as one blob [nodes | index | prefix ‖ keys]; staged into
  // LDS by k_match when blob_words != 0 (it fits CFG_LDS_WORDS)
  const uint8_t* blob;
  uint32_t blob_words, idx_word, key_word;
};
constexpr uint32_t CFG_LDS_WORDS = 12288 / 4;

// Raw request batch on the device (rl_request_batch).
struct ReqDev {
  uint32_t n_req, n_desc, n_ent;
  uint32_t dom_total, desc_total;  // bytes behind dom / desc (offsets are checked against them)
  const uint8_t* dom;
  const uint32_t* dom_off;
  const uint32_t* hits;
  const uint32_t* req;
  const uint32_t* ent_first;
  const uint32_t* desc_off;
  const uint8_t* desc;
  const uint16_t* klen;
  const uint16_t* vlen;
  const uint8_t* ovf;
  const uint32_t* ov_rpu;
  const uint8_t* ov_unit;
  const uint32_t* ov_rule;
};

// The compacted DoLimit batch the matched descriptors are written into.
struct PackOut {
  uint8_t* stem;
  uint32_t* off;
  uint32_t* req;
  uint8_t* unit;
  uint8_t* flags;
  uint32_t* limit;
  uint32_t* hits;
  uint32_t* rule;
  uint32_t stem_cap;
};

// Per-descriptor match results.
struct MatchBuf {
  unsigned long long* v;     // [2n]: (matched << 40) | stem bytes, then its inclusive scan
  uint32_t* kind;            // rl_match | unit << 8 | shadow << 16
  uint32_t* rpu;
  uint32_t* rule;
  uint32_t* count;           // [0] matched descriptors, [1] stem bytes, [2] error bits
};

// The service's per-descriptor answer (rl_request_result, device arrays).
struct ReqOutDev {
  uint8_t* code;
  uint32_t* rem;
  uint32_t* reset;
  uint8_t* match;
  uint32_t* rule;
  uint32_t* rpu;
  uint8_t* unit;
};

// The per-request verdict (rl_request_verdict) on the device: its inputs are
// the per-descriptor answers, its scratch and outputs one carved block
//   [inv_min u64 nq | over u32 nq | pad | shadow u64 | min_desc, limit,
//    remaining, reset u32 nq each | code u8 nq | flags u8 nq]
// The accumulators (up to and including the shadow count) are zeroed on the
// stream.
struct VerdictDev {
  uint32_t n_req, n_desc, opts;
  const uint32_t* req;
  const uint8_t* match;
  const uint8_t* code;
  const uint32_t* rem;
  const uint32_t* reset;
  const uint32_t* rpu;
  unsigned long long* inv_min;  // ~min((remaining << 32) | d) over the limited descriptors; 0 = none
  uint32_t* over;               // max(d + 1) over the OVER_LIMIT descriptors; 0 = none
  unsigned long long* shadow;   // [1] requests that global shadow mode turned into OK
  uint32_t* o_min;
  uint32_t* o_limit;
  uint32_t* o_rem;
  uint32_t* o_reset;
  uint8_t* o_code;
  uint8_t* o_flags;
};

struct VerdictLayout {
  size_t inv_min, over, shadow, o_min, o_limit, o_rem, o_reset, o_code, o_flags, bytes;
  size_t acc_bytes() const { return shadow + 8; }  // zeroed before the kernels
};
inline VerdictLayout verdict_layout(uint32_t nq) {
  VerdictLayout L;
  const size_t q = nq;
  L.inv_min = 0;
  L.over = 8 * q;
  L.shadow = (12 * q + 7) & ~(size_t)7;
  L.o_min = L.shadow + 8;
  L.o_limit = L.o_min + 4 * q;
  L.o_rem = L.o_limit + 4 * q;
  L.o_reset = L.o_rem + 4 * q;
  L.o_code = L.o_reset + 4 * q;
  L.o_flags = L.o_code + q;
  L.bytes = L.o_flags + q;
  return L;
}

constexpr uint32_t MATCH_ERR_REQ = 1, MATCH_ERR_CAP = 2;
constexpr uint32_t MATCH_ERR_UNPACK = 4;  // k_unpack_requests: an index entry or override that does not match the batch

__host__ __device__ inline uint64_t cfg_hash(int32_t parent, const uint8_t* p, uint32_t len) {
  uint64_t h = 0xcbf29ce484222325ull ^ ((uint64_t)(uint32_t)(parent + 1) * 0x9E3779B97F4A7C15ull);
  for (uint32_t i = 0; i < len; i++) {
    h ^= p[i];
    h *= 0x100000001b3ull;
  }
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return h;
}

// Enqueue: match every descriptor, scan, compact. Scan temp storage is
// `tmp` (tmp_bytes from match_scan_bytes).
size_t match_scan_bytes(uint32_t n);
void launch_match(const CfgDev& cfg, const ReqDev& r, const MatchBuf& m, const PackOut& o, void* tmp,
                  size_t tmp_bytes, hipStream_t st);
void launch_match_expand(const ReqDev& r, const MatchBuf& m, const uint8_t* code, const uint32_t* rem,
                         const uint32_t* reset, const ReqOutDev& out, hipStream_t st);
// A one-buffer request batch (rl_request_batch_packed; buf = the device copy
// of its buffer) -> the arrays of ReqDev that do not cross the link: dom_off
// [nq + 1], req [n], ent_first and desc_off [n + 1], the 64-bit clocks, and
// the dense override arrays scattered from the sparse list (zeroed by the
// caller on the stream when n_overrides != 0, else unused). The totals come
// from the host buffer's last index entry (already checked against the batch's
// sizes). A tile or override that does not match sets MATCH_ERR_UNPACK in *err.
void launch_unpack_requests(const rl_request_batch_packed& pb, const uint8_t* buf, uint32_t* dom_off, int64_t* now,
                            uint32_t* req, uint32_t* ent_first, uint32_t* desc_off, uint8_t* ovf, uint32_t* ov_rpu,
                            uint8_t* ov_unit, uint32_t* ov_rule, uint32_t* err, hipStream_t st);
// Enqueue the verdict over per-descriptor answers already on the device
// (v.req non-decreasing and < v.n_req): zeroes the accumulators at `block`
// (verdict_layout(v.n_req), whose pointers v holds), then k_verdict and
// k_verdict_final.
hipError_t launch_verdict(const VerdictDev& v, uint8_t* block, hipStream_t st);
// ---- serialized RateLimitRequest payloads parsed on the device (rl_wire.hip)
constexpr uint32_t MATCH_ERR_WIRE = 8;  // k_wire_emit: a message's re-walk left its counted share
// error bits of the count stage (WireDev::cnt[4])
constexpr uint32_t WIRE_ERR_OFF = 1;    // msg_off decreasing or past msgs_bytes
constexpr uint32_t WIRE_ERR_SUM = 2;    // a batch total does not fit 32 bits

// The override stats keys interned on the device (rl_override_rules_enable):
// descriptorKey bytes -> a dense index (rule id - first_rule). Open addressing
// over `slots`: 0 empty, else tag (the hash's high word) << 32 | low word, the
// low word being index + 1 once published, OV_BUSY while its one inserter
// (k_wire_intern) writes the key, OV_DEAD for a slot whose insert found no id
// or arena space (never reused: probes pass it). A key's bytes, offset and
// length are written once, before the slot word is published (agent-scope
// release); readers match only published words (acquire) and confirm the full
// bytes. Probes are bounded by OV_PROBE.
constexpr uint32_t OV_BUSY = 0xFFFFFFFFu, OV_DEAD = 0xFFFFFFFEu, OV_NONE = 0xFFFFFFFFu;
constexpr uint32_t OV_PROBE = 64, OV_KEY_MAX = 65535u;
// Every override's key repeats the message's domain, so a long domain in front of many small overrides
// makes a lane hash far more bytes than the message holds. A message whose overrides x (domain bytes + 1)
// exceed OV_WORK_X times its own length stays deferred: a lane's work is linear in its payload.
constexpr uint32_t OV_WORK_X = 16;
struct OvDev {
  unsigned long long* slots;  // [mask + 1]
  uint32_t mask;
  uint32_t first_rule, capacity;
  uint32_t arena_cap;         // bytes behind arena (< 2^32)
  uint32_t* koff;             // [capacity] a key's first byte in arena
  uint32_t* klen;             // [capacity]
  uint8_t* arena;
  // [0] ids handed out << 32 | arena bytes used (one word: both or neither are taken), [1] deferred_full
  unsigned long long* ctr;
  uint64_t k0, k1;            // the ctx's hash key
};

// A wire batch on the device: the sections of the copied buffer and the
// count stage's arrays (sized by the request count alone).
struct WireDev {
  uint32_t n_req, tiles, msgs_bytes;
  const uint32_t* msg_off;  // [n_req + 1]
  const uint32_t* now32;    // [n_req]
  const uint8_t* msgs;
  uint4* reqw;     // [n_req] {descriptors | status << 24, entries, domain bytes, entry bytes}; zero counts unless OK
  uint4* tsum;     // [tiles] the tiles' sums of those four
  uint4* index;    // [tiles + 1] their exclusive scan: rl_request_batch_packed's tile index
  uint32_t* cnt;   // [8] the totals {descriptors, entries, domain bytes, entry bytes}, error bits
  uint8_t* status;        // [n_req] rl_wire_status
  uint32_t* desc_first;   // [n_req + 1]
  // enabled ctxs only (cnt[5]: messages that stayed OK with an override, cnt[6]: entries of miss)
  uint32_t n_rules;       // override rule ids must stay below it
  uint32_t* miss;         // [n_req] messages with an override key the count stage did not find
};

// What k_wire_emit writes: ReqDev's arrays and the clocks. The dense override
// arrays (null unless the batch carries overrides; zeroed on the stream) are
// written for the descriptors with `limit` alone.
struct WireOut {
  uint4 tot;  // the count stage's totals, capacity-checked on the host
  uint32_t* dom_off;
  uint32_t* hits;
  int64_t* now;
  uint32_t* req;
  uint32_t* ent_first;
  uint32_t* desc_off;
  uint16_t* klen;
  uint16_t* vlen;
  uint8_t* dom;
  uint8_t* desc;
  uint32_t* err;  // MatchBuf::count + 2
  uint8_t* ovf;
  uint32_t* ov_rpu;
  uint8_t* ov_unit;
  uint32_t* ov_rule;
};

// k_wire_count per tile, then the scan over the tiles (index, totals, desc_first[n_req]).
// ov (enabled ctxs): messages with `limit` are looked up in the intern table
// by the count kernel; k_wire_intern (one workgroup; the caller orders it after
// the previous batch's by `ov_order`, recorded again behind it) inserts the
// keys it missed and defers what it cannot serve, before the scan.
void launch_wire_count(const WireDev& w, hipStream_t st, const OvDev* ov = nullptr, hipEvent_t ov_order = nullptr,
                       bool ov_wait = false);
// ov: the batch carries overrides (o.ovf and its kin are set).
void launch_wire_emit(const WireDev& w, const WireOut& o, hipStream_t st, const OvDev* ov = nullptr);
// overall_code[q] = 0 where status[q] != RL_WIRE_OK
void launch_wire_code(const uint8_t* status, uint8_t* o_code, uint32_t n_req, hipStream_t st);

// ---- serialized RateLimitResponse payloads written on the device (rl_resp.hip)
// The answers and the verdict of one batch (device arrays) and the response
// staging: soff and resp_off hold the sizes first and their exclusive scans
// after launch_respond's scans. bytes is 4-byte aligned, cap bytes long.
struct RespDev {
  uint32_t n_req, n_desc, cap;
  const uint32_t* req;          // [n_desc] each descriptor's request
  const uint32_t* desc_first;   // [n_req + 1]
  const uint8_t* status;        // [n_req] rl_wire_status, or null: every request RL_WIRE_OK
  const uint8_t* code;
  const uint32_t* rem;
  const uint32_t* reset;
  const uint8_t* match;
  const uint32_t* rpu;
  const uint8_t* unit;
  const uint8_t* o_code;        // the verdict's outputs
  const uint32_t* o_min;
  const uint32_t* o_limit;
  const uint32_t* o_rem;
  const uint32_t* o_reset;
  uint32_t* soff;               // [n_desc + 1] status bytes before each descriptor
  uint32_t* resp_off;           // [n_req + 1]
  uint8_t* bytes;
  void* tmp;                    // the scans' temp storage (resp_scan_bytes)
  size_t tmp_bytes;
};
struct RespLayout {
  size_t soff, resp_off, tmp, bytes, total;
  size_t tmp_bytes, cap;
};
// The staging of a batch of nq requests over n descriptors whose responses take at most `bound` bytes.
RespLayout resp_layout(uint32_t nq, uint32_t n, uint64_t bound);
// Enqueue: the size pass, the two scans, the emit pass. n_req != 0.
hipError_t launch_respond(const RespDev& r, const rlresp::Format& fmt, hipStream_t st);
// Enqueue the copy of bytes[0, min(resp_off[n_req], cap)) to dst (device-visible host memory).
void launch_respond_to_host(const RespDev& r, uint8_t* dst, hipStream_t st);

VerdictDev verdict_view(uint32_t n_req, uint32_t n_desc, uint32_t opts, const uint32_t* req, const uint8_t* match,
                        const uint8_t* code, const uint32_t* rem, const uint32_t* reset, const uint32_t* rpu,
                        uint8_t* block);

}  // namespace rl
