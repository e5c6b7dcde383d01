/* requests_packed_san.c — rl_request_batch_pack (ratelimit_amd/csrc/rl_pack.cpp)
 * under AddressSanitizer + UndefinedBehaviorSanitizer
 * (tests/test_requests_packed_cpu.py builds both with -fsanitize=address,undefined
 * -fno-sanitize-recover=all, like san_run.c). Every input array is a heap block
 * of exactly its size, so a read past an array's end is a finding. Drives the
 * converter over well-formed batches of several shapes, truncated
 * capacities of each, and the malformed inputs it must refuse; after a refusal
 * the output buffer must still hold its fill. Prints "OK <calls>" and exits 0;
 * any mismatch exits 1, any finding aborts. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ratelimit_hip.h"

typedef struct {
  rl_request_batch b;
  uint8_t *dom, *desc, *ovf, *ovu;
  uint32_t *dom_off, *hits, *req, *ent, *doff, *ovr, *ovrule;
  int64_t* now;
  uint16_t *kl, *vl;
} Batch;

static uint32_t rnd_state = 12345u;
static uint32_t rnd(void) {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}

static void* exact(size_t bytes) {  /* (a zero-size array is still a distinct block) */
  void* p = malloc(bytes ? bytes : 1);
  if (!p) exit(2);
  memset(p, 0, bytes ? bytes : 1);
  return p;
}

/* nq requests; request q has nd(q) descriptors, each 0-3 entries; overrides on every ov_every-th descriptor */
static Batch make(uint32_t nq, uint32_t big_request, uint32_t big_n, uint32_t ov_every) {
  Batch B;
  memset(&B, 0, sizeof B);
  uint32_t n = 0, ne = 0, q, d, e;
  uint32_t* nd = (uint32_t*)exact(4u * nq);
  for (q = 0; q < nq; q++) {
    nd[q] = q == big_request ? big_n : rnd() % 4;
    n += nd[q];
  }
  uint32_t* cnt = (uint32_t*)exact(4u * n);
  for (d = 0; d < n; d++) {
    cnt[d] = rnd() % 4;
    ne += cnt[d];
  }
  B.kl = (uint16_t*)exact(2u * ne);
  B.vl = (uint16_t*)exact(2u * ne);
  uint64_t bytes = 0, dbytes = 0;
  for (e = 0; e < ne; e++) {
    B.kl[e] = (uint16_t)(rnd() % 9);
    B.vl[e] = (uint16_t)(rnd() % 7);
    bytes += B.kl[e] + B.vl[e] + 2u;
  }
  B.dom_off = (uint32_t*)exact(4u * (nq + 1));
  B.hits = (uint32_t*)exact(4u * nq);
  B.now = (int64_t*)exact(8u * nq);
  for (q = 0; q < nq; q++) {
    dbytes += rnd() % 12;
    B.dom_off[q + 1] = (uint32_t)dbytes;
    B.hits[q] = rnd() % 9;
    B.now[q] = 1700000000 + (int64_t)q;
  }
  B.dom = (uint8_t*)exact(dbytes);
  for (e = 0; e < dbytes; e++) B.dom[e] = (uint8_t)('a' + rnd() % 26);
  B.desc = (uint8_t*)exact(bytes);
  for (e = 0; e < bytes; e++) B.desc[e] = (uint8_t)('A' + rnd() % 26);
  B.req = (uint32_t*)exact(4u * n);
  B.ent = (uint32_t*)exact(4u * (n + 1));
  B.doff = (uint32_t*)exact(4u * (n + 1));
  d = 0;
  for (q = 0; q < nq; q++)
    for (e = 0; e < nd[q]; e++) B.req[d++] = q;
  uint32_t ef = 0, bo = 0;
  for (d = 0; d < n; d++) {
    for (e = 0; e < cnt[d]; e++) bo += B.kl[ef + e] + B.vl[ef + e] + 2u;
    ef += cnt[d];
    B.ent[d + 1] = ef;
    B.doff[d + 1] = bo;
  }
  if (ov_every) {
    B.ovf = (uint8_t*)exact(n);
    B.ovu = (uint8_t*)exact(n);
    B.ovr = (uint32_t*)exact(4u * n);
    B.ovrule = (uint32_t*)exact(4u * n);
    for (d = 0; d < n; d += ov_every) {
      B.ovf[d] = 1;
      B.ovu[d] = (uint8_t)(1 + d % 4);
      B.ovr[d] = d * 3u;
      B.ovrule[d] = d % 5;
    }
  }
  free(nd);
  free(cnt);
  B.b.n_requests = nq;
  B.b.n_descriptors = n;
  B.b.n_entries = ne;
  B.b.n_rules = 5;
  B.b.domain_bytes = B.dom;
  B.b.domain_off = B.dom_off;
  B.b.now = B.now;
  B.b.hits = B.hits;
  B.b.req_idx = B.req;
  B.b.entry_first = B.ent;
  B.b.desc_off = B.doff;
  B.b.desc_bytes = B.desc;
  B.b.key_len = B.kl;
  B.b.value_len = B.vl;
  B.b.override_flags = B.ovf;
  B.b.override_rpu = B.ovr;
  B.b.override_unit = B.ovu;
  B.b.override_rule = B.ovrule;
  return B;
}

static void destroy(Batch* B) {
  free(B->dom); free(B->desc); free(B->ovf); free(B->ovu); free(B->dom_off); free(B->hits); free(B->req);
  free(B->ent); free(B->doff); free(B->ovr); free(B->ovrule); free(B->now); free(B->kl); free(B->vl);
}

static unsigned long calls = 0;

static void die(const char* what, int line) {
  fprintf(stderr, "requests_packed_san: %s (line %d)\n", what, line);
  exit(1);
}
#define CHECK(x) do { if (!(x)) die(#x, __LINE__); } while (0)

/* one call into a fresh exact-size buffer of `cap` bytes filled with 0xA5; a refusal leaves the fill */
static int pack(const rl_request_batch* b, uint64_t cap, rl_request_batch_packed* p) {
  uint8_t* buf = (uint8_t*)exact((size_t)cap);
  uint64_t i;
  memset(buf, 0xA5, (size_t)(cap ? cap : 1));
  const int rc = rl_request_batch_pack(b, buf, cap, p);
  calls++;
  if (rc != RL_OK)
    for (i = 0; i < cap; i++) CHECK(buf[i] == 0xA5);
  free(buf);
  return rc;
}

static void well_formed(const rl_request_batch* b) {
  rl_request_batch_packed p;
  uint64_t need, cap;
  memset(&p, 0, sizeof p);
  CHECK(rl_request_batch_pack(b, NULL, 0, &p) == RL_E_CAPACITY);
  need = p.buf_bytes;
  CHECK(need >= 16 && need % 4 == 0);
  for (cap = 0; cap < need; cap += (need > 256 ? need / 61 + 1 : 1)) {  /* every capacity of a small batch, ~60 of a large one */
    memset(&p, 0, sizeof p);
    CHECK(pack(b, cap, &p) == RL_E_CAPACITY && p.buf_bytes == need);
  }
  CHECK(pack(b, need - 1, &p) == RL_E_CAPACITY);
  CHECK(pack(b, need, &p) == RL_OK && p.buf_bytes == need && p.n_descriptors == b->n_descriptors);
}

static void refused(const rl_request_batch* b) {
  rl_request_batch_packed p;
  memset(&p, 0, sizeof p);
  CHECK(pack(b, 1u << 20, &p) == RL_E_INVALID);
  CHECK(rl_request_batch_pack(b, NULL, 0, &p) == RL_E_INVALID);
}

int main(void) {
  const uint32_t shapes[][4] = {{0, 0, 0, 0}, {1, 9, 0, 0}, {255, 9999, 0, 3}, {256, 0, 0, 1}, {257, 256, 300, 7},
                                {513, 255, 300, 5}, {40, 3, 1000, 0}};
  size_t s;
  for (s = 0; s < sizeof shapes / sizeof shapes[0]; s++) {
    Batch B = make(shapes[s][0], shapes[s][1], shapes[s][2], shapes[s][3]);
    well_formed(&B.b);
    destroy(&B);
  }
  /* the malformed inputs, each on a fresh well-formed batch */
  {
    Batch B = make(300, 7, 40, 4);
    const uint32_t n = B.b.n_descriptors, nq = B.b.n_requests;
    uint32_t save;
    int64_t t;
    CHECK(n > 100);
    save = B.dom_off[5]; B.dom_off[5] = B.dom_off[6] + 1; refused(&B.b); B.dom_off[5] = save;       /* non-monotone */
    save = B.dom_off[0]; B.dom_off[0] = 1; refused(&B.b); B.dom_off[0] = save;
    save = B.ent[9]; B.ent[9] = B.ent[10] + 1; refused(&B.b); B.ent[9] = save;
    save = B.ent[n]; B.ent[n] = save + 1; refused(&B.b); B.ent[n] = save;                              /* past n_entries */
    save = B.doff[9]; B.doff[9] = B.doff[8] ? B.doff[8] - 1 : B.doff[10] + 1; refused(&B.b); B.doff[9] = save;
    save = B.doff[n]; B.doff[n] = save + 1; refused(&B.b); B.doff[n] = save;                           /* span != sum */
    save = B.req[20]; B.req[20] = nq; refused(&B.b); B.req[20] = save;
    save = B.req[20]; B.req[20] = B.req[19] ? B.req[19] - 1 : nq + 3; refused(&B.b); B.req[20] = save;  /* decreasing */
    if (B.b.n_entries) { B.kl[0]++; refused(&B.b); B.kl[0]--; }
    t = B.now[3]; B.now[3] = -1; refused(&B.b); B.now[3] = (int64_t)1 << 32; refused(&B.b); B.now[3] = t;
    { const uint32_t* keep = B.b.override_rpu; B.b.override_rpu = NULL; refused(&B.b); B.b.override_rpu = keep; }
    { const uint32_t* keep = B.b.domain_off; B.b.domain_off = NULL; refused(&B.b); B.b.domain_off = keep; }
    refused(NULL);
    well_formed(&B.b);  /* (restored) */
    destroy(&B);
  }
  {
    /* a request of 65536 descriptors, a domain of 65536 bytes, a descriptor of 65536 entries */
    Batch B = make(3, 1, 65536, 0);
    refused(&B.b);
    destroy(&B);
    B = make(3, 1, 65535, 0);
    well_formed(&B.b);
    destroy(&B);
  }
  {
    rl_request_batch b;
    rl_request_batch_packed p;
    uint32_t dom_off[2] = {0, 65536}, zero2[2] = {0, 0}, hits = 1;
    int64_t now = 5;
    uint8_t* dom = (uint8_t*)exact(65536);
    memset(&b, 0, sizeof b);
    b.n_requests = 1;
    b.domain_bytes = dom;
    b.domain_off = dom_off;
    b.now = &now;
    b.hits = &hits;
    b.entry_first = zero2;
    b.desc_off = zero2;
    refused(&b);
    dom_off[1] = 65535;
    CHECK(pack(&b, 1u << 20, &p) == RL_OK);
    free(dom);
  }
  {
    rl_request_batch b;
    uint32_t dom_off[2] = {0, 0}, ent[2] = {0, 65536}, doff[2] = {0, 65536u * 2u}, hits = 1, req = 0;
    int64_t now = 5;
    uint16_t* z = (uint16_t*)exact(2u * 65536u);
    uint8_t* bytes = (uint8_t*)exact(65536u * 2u);
    memset(&b, 0, sizeof b);
    b.n_requests = 1;
    b.n_descriptors = 1;
    b.n_entries = 65536;
    b.domain_off = dom_off;
    b.now = &now;
    b.hits = &hits;
    b.req_idx = &req;
    b.entry_first = ent;
    b.desc_off = doff;
    b.desc_bytes = bytes;
    b.key_len = z;
    b.value_len = z;
    refused(&b);
    free(z);
    free(bytes);
  }
  printf("OK %lu\n", calls);
  return 0;
}
