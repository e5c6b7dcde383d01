"""The 8-byte tile record between k_part and the bucket kernels
({sort key, index | hits9 << 23}, ratelimit_amd/csrc/rl_tile.h), checked for
exact equality against the C oracle with every limit at 2^32 - 1, so that the
counts (and with them every descriptor's hits) show in limit_remaining:

* k_part's tile edges: batch sizes around one and two tiles of 4096, a
  duplicated key straddling each tile boundary and one inside a tile;
* the hits escape: hits9 = 511 sends the reader to the batch's hits array, for
  keys seen once and runs of 2 and 3 with hits on both sides of 511;
* the bucket capacity: one key 2048 times (k_bucket at CAP), 2049 times (the
  large-bucket kernels) and 3000 times with hits of 100000 among 1200 other
  keys (a hot key sampled by k_bucket and placed chunk by chunk by
  k_big_count / k_big_place, hits read through the escape), under both shapes
  of the large-bucket cue;
* the large buckets' one-workgroup fallback: 2M descriptors of mostly distinct
  keys, about half of the 1024 buckets over CAP with no hot key, so
  bucket_peel gives up and bucket_lsd sorts them through HBM, with hits of
  510, 511 and 70000 on keys seen once and on duplicated ones;
* a routed owner batch (two loopback ranks) whose duplicates carry hits of 511
  and more: the escape then reads the owner's own copy of the hits."""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from ratelimit_amd import workloads as W
from ratelimit_amd.limiter import Backend

pytestmark = pytest.mark.gpu

NOW0 = W.NOW0
FIELDS = ("code", "limit_remaining", "reset_s", "stats")
U32 = 0xFFFFFFFF
PART_TILE = 4096  # k_part's tile


def _batch(ids, now, hits):
    """One descriptor per request: key ids[i] (unit MINUTE, limit 2^32 - 1, rule 0) with hits[i]."""
    ids = np.asarray(ids, np.int64)
    n = ids.size
    stems, L = W._fixed_stems(b"tile_key_k", ids, 10, b"_min_")
    return {
        "stem_bytes": stems.reshape(-1),
        "stem_off": (np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32),
        "now": np.full(n, now, np.int64),
        "req_idx": np.arange(n, dtype=np.uint32),
        "unit": np.full(n, 2, np.uint8),
        "flags": np.zeros(n, np.uint8),
        "limit": np.full(n, U32, np.uint32),
        "hits": np.asarray(hits, np.uint32),
        "rule_id": np.zeros(n, np.uint32),
    }, n, n, 1


def _oracle(batches):
    co = c_oracle.COracle(0.8, False)
    try:
        return [co.do_limit(*b) for b in batches]
    finally:
        co.close()


def _check(batches, want, **kw):
    cfg = dict(table_slots=1 << 16, max_batch=1 << 14, max_rules=8)
    cfg.update(kw)
    be = Backend(0.8, False, **cfg)
    try:
        for i, (a, n, nq, nr) in enumerate(batches):
            g = be.do_limit_arrays(a, n, nq, nr)
            for k in FIELDS:
                assert np.array_equal(g[k], want[i][k]), "batch %d: %s differs at %s" % (
                    i, k, np.nonzero(np.asarray(g[k]) != np.asarray(want[i][k]))[0][:8])
    finally:
        be.close()


# --------------------------------------------------------------------------- tile edges
@functools.lru_cache(maxsize=None)
def _edges(n):
    """n distinct keys in arrival order, except one pair inside the first tile
    (positions 10 and 20) and one pair straddling each tile boundary
    (positions 4096 t - 1 and 4096 t); hits 1..7 by position. Twice, one clock
    apart: the second batch counts on top of the first."""
    ids = 1000 + np.arange(n)
    if n > 20:
        ids[20] = ids[10]
    for edge in range(PART_TILE, n, PART_TILE):
        ids[edge] = ids[edge - 1]
    hits = 1 + np.arange(n) % 7
    bs = [_batch(ids, NOW0, hits), _batch(ids[::-1], NOW0 + 1, hits)]
    return bs, _oracle(bs)


@pytest.mark.parametrize("n", [1, 255, 256, 4095, 4096, 4097, 8193])
def test_gpu_tile_edges_vs_c_oracle(n):
    bs, want = _edges(n)
    _check(bs, want)


# --------------------------------------------------------------------------- the hits escape
ESC_HITS = (0, 1, 510, 511, 512, 65535, U32)


@functools.lru_cache(maxsize=None)
def _escape():
    """Per hits value: a key seen once, a run of 2 and a run of 3, all with
    that value, among 300 keys seen once with hits 1, and one run of 3 mixing
    510, 511 and 2^32 - 1; shuffled. Two batches one clock apart."""
    rng = np.random.default_rng(511)
    ids, hits = [], []
    for k, h in enumerate(ESC_HITS):
        for rep, key in ((1, 10 * k), (2, 10 * k + 1), (3, 10 * k + 2)):
            ids += [key] * rep
            hits += [h] * rep
    ids += [900, 900, 900]
    hits += [510, 511, U32]
    ids += list(1000 + np.arange(300))
    hits += [1] * 300
    ids, hits = np.asarray(ids), np.asarray(hits, np.uint32)
    bs = []
    for k in range(2):
        p = rng.permutation(ids.size)
        bs.append(_batch(ids[p], NOW0 + k, hits[p]))
    return bs, _oracle(bs)


def test_gpu_hits_escape_singletons_and_runs_vs_c_oracle():
    bs, want = _escape()
    rem = np.concatenate([w["limit_remaining"] for w in want])
    assert len(np.unique(rem)) > len(ESC_HITS), "the counts show in limit_remaining"
    _check(bs, want)


# --------------------------------------------------------------------------- bucket capacity
@functools.lru_cache(maxsize=None)
def _capacity(kind):
    """Three equal batches one clock apart (the large-bucket cue, when on, is
    raised by the first and seen by the later ones)."""
    rng = np.random.default_rng(2048)
    if kind == "cap":  # one bucket of exactly BkSmall::CAP elements: k_bucket's own path
        ids, hits = np.full(2048, 7), 1 + np.arange(2048) % 5
    elif kind == "over":  # one more: queued for the large-bucket kernels
        ids, hits = np.full(2049, 7), 1 + np.arange(2049) % 5
    else:  # a hot key with escaped hits among 1200 keys seen once
        ids = rng.permutation(np.r_[np.full(3000, 7), 1000 + np.arange(1200)])
        hits = np.where(ids == 7, 100000, 1 + np.arange(ids.size) % 600)
    bs = [_batch(ids, NOW0 + k, hits) for k in range(3)]
    return bs, _oracle(bs)


@pytest.mark.parametrize("cue", ["0", None], ids=["full_grids", "cue"])
@pytest.mark.parametrize("kind", ["cap", "over", "hot"])
def test_gpu_bucket_capacity_vs_c_oracle(monkeypatch, kind, cue):
    if cue is None:
        monkeypatch.delenv("RL_BIG_CUE", raising=False)
    else:
        monkeypatch.setenv("RL_BIG_CUE", cue)
    bs, want = _capacity(kind)
    _check(bs, want)


# --------------------------------------------------------------------------- the one-workgroup fallback
@functools.lru_cache(maxsize=None)
def _fallback():
    """2^20 requests (two stems each: 2^21 descriptors, 2048 per bucket on
    average, so about half the buckets exceed BkSmall::CAP); every 20th
    request repeats its neighbour's tenant (runs of two, 5 % of the batch, so
    no key is sampled three times in a bucket: no hot key, and bucket_peel
    hands the bucket to bucket_lsd). Hits are drawn from 1, 510, 511 and 70000
    per request, so escaped hits fall on keys seen once and on either or both
    elements of the runs."""
    nq = 1 << 20
    rng = np.random.default_rng(4097)
    t = rng.permutation(nq) + 5000
    t[20::20] = t[19:-1:20]
    h = np.asarray([1, 510, 511, 70000], np.uint32)[rng.integers(0, 4, nq)]
    a, n, q, nr = W.c1_batch(t, NOW0, h)
    a["limit"][:] = U32
    bs = [(a, n, q, nr)]
    return bs, _oracle(bs)


def test_gpu_large_bucket_fallback_reads_escaped_hits_vs_c_oracle():
    bs, want = _fallback()
    assert len(np.unique(want[0]["limit_remaining"])) >= 8, "the counts show in limit_remaining"
    n = bs[0][1]
    _check(bs, want, table_slots=2 * n, max_batch=n)


# --------------------------------------------------------------------------- routed owner batch
def test_gpu_routed_owner_batch_reads_escaped_hits_vs_c_oracle():
    """Two loopback ranks: every owner batch is a routed one (wire records and
    the own chunk), so k_part and the escape read Scratch::hit_a."""
    from test_gpu_loopback import _check as check_world, run_world
    rng = np.random.default_rng(23)
    batches = []
    for k in range(2):
        t = rng.permutation(np.r_[np.repeat(np.arange(40), 3), 100 + np.arange(400)])
        h = np.where(t < 40, np.asarray(ESC_HITS[2:], np.uint32)[t % 5], 1 + t % 9).astype(np.uint32)
        a, n, nq, nr = W.c1_batch(t, NOW0 + k, h)
        a["limit"][:] = U32
        batches.append((a, n, nq, nr))
    cfg = (0.8, False, False)
    out = run_world(2, batches, cfg)
    for r in range(2):
        assert out[r][0] == "ok", out[r][1]
    check_world(out, batches, cfg, 2)
