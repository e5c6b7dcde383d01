"""k_bucket's shapes: bucket sizes and duplicate counts across every strip
boundary, and the host's cue for the keys-seen-once list.

k_bucket's four waves hold strips of 64 positions per item, so the code a
bucket runs changes with its size S (while it looks for duplicated keys) and
with the number M of duplicated elements (in its sort) at every multiple of 64
and 256: one wave ranks M <= 64 by comparisons, lds_sort3 sorts more, and a
bucket over BkSmall::CAP = 2048 goes to the large-bucket kernels. It reserves
its sorted block, run ids and dup-run entries in one round before the sort,
from the count of duplicated keys its LDS hash gives. The keys-seen-once list
(Scratch::uniq) is built only while the host's cue says recent batches were
sparse (RL_LIST_CUE: 0 always, 1 the cue, 2 never); a batch answers the same
with and without it. Every answer must equal the C oracle's."""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from ratelimit_amd import workloads as W
from ratelimit_amd.limiter import Backend
import magnitude as M

pytestmark = pytest.mark.gpu

NOW0 = W.NOW0
FIELDS = ("code", "limit_remaining", "reset_s", "stats")
PART_DIGITS = 1024  # k_bucket's buckets: the sort key's top 10 bits


def _oracle(batches, lc, ps=False):
    co = c_oracle.COracle(0.8, lc, ps)
    try:
        return [co.do_limit(*b) for b in batches]
    finally:
        co.close()


def _check(batches, want, lc, ps=False, isolate=False, **kw):
    cfg = dict(table_slots=1 << 17, max_batch=1 << 16, max_rules=8)
    cfg.update(kw)
    be = Backend(0.8, lc, ps, **cfg)
    try:
        for i, (a, n, nq, nr) in enumerate(batches):
            g = be.do_limit_arrays(a, n, nq, nr, isolate=isolate)
            if isolate:
                assert not g["status"].any(), "batch %d: statuses %s" % (i, np.unique(g["status"]))
            for k in FIELDS:
                assert np.array_equal(g[k], want[i][k]), "batch %d: %s differs at %s" % (
                    i, k, np.nonzero(np.asarray(g[k]) != np.asarray(want[i][k]))[0][:8])
    finally:
        be.close()


# --------------------------------------------------------------------------- bucket sizes
@functools.lru_cache(maxsize=None)
def _uniform(mu):
    """n = 1024 * mu descriptors of distinct tenants (every sort key seen once,
    bucket sizes binomial around mu: each of mu - 1, mu, mu + 1 in about
    1024 / sqrt(2 pi mu) >= 9 buckets), twice, one clock apart: the second
    pass finds the minute slots live and rolls the second ones."""
    nq = PART_DIGITS * mu // 2
    rng = np.random.default_rng(1000 + mu)
    t = rng.permutation(nq) + 10 * mu
    h = rng.integers(1, 9, nq).astype(np.uint32)
    bs = [W.c1_batch(t, NOW0, h), W.c1_batch(t[::-1], NOW0 + 1, h)]
    return bs, _oracle(bs, False)


@pytest.mark.parametrize("mu", [64, 256, 512, 1024, 2048])
def test_gpu_bucket_sizes_across_strip_boundaries_vs_c_oracle(mu):
    """Mean bucket sizes of 64 (one item on one wave), 256, 512 (one wave's
    whole strip), 1024 (two waves') and CAP = 2048, where about half the
    buckets go to the large-bucket kernels."""
    bs, want = _uniform(mu)
    n = bs[0][1]
    _check(bs, want, False, table_slots=max(1 << 17, 2 * n), max_batch=max(1 << 16, n))


# --------------------------------------------------------------------------- duplicate counts
DUP_COUNTS = (2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)


@functools.lru_cache(maxsize=None)
def _dups(hits, lc):
    """Hot tenant c repeats exactly DUP_COUNTS[c] times (its second and its
    minute stem: one run of that length each, in two buckets) over 4000
    distinct tenants (~27 descriptors per bucket): M = the count, or a few more
    where another run shares the bucket; 2047 and 2048 with the background go
    over CAP. Two batches one clock apart."""
    rng = np.random.default_rng(77)
    hot = np.concatenate([np.full(c, 10 + k) for k, c in enumerate(DUP_COUNTS)])
    bs = []
    for k in range(2):
        t = rng.permutation(np.r_[hot, 1000 + np.arange(4000)])
        bs.append(W.c1_batch(t, NOW0 + k, np.full(t.size, hits, np.uint32)))
    return bs, _oracle(bs, lc)


@pytest.mark.parametrize("lc", [False, True])
@pytest.mark.parametrize("hits", [0, 1, 5])
def test_gpu_duplicate_counts_across_sort_boundaries_vs_c_oracle(hits, lc):
    """Runs of 2 .. 2048: the one-wave rank against lds_sort3 (64 / 65), the
    steps of the sort's strips (256 / 257, 512 / 513, 1024 / 1025) and the
    hand-off at CAP, each run's ids and dup-run entry reserved before the
    sort; with hits of 5 the long runs cross both limits."""
    bs, want = _dups(hits, lc)
    codes = np.concatenate([w["code"] for w in want])
    if hits == 5:
        assert len(np.unique(codes)) > 1, "the long runs cross their limits"
    _check(bs, want, lc)


# --------------------------------------------------------------------------- the cue
CUE_MODES = ["0", "2", None]  # RL_LIST_CUE: list always built, never built, the default (the cue)


def _cue_batches(dense_tenants, sparse_rpb, seed):
    """Sparse batches (Zipf over 300 tenants: few keys seen once) between dense
    ones (distinct tenants): two sparse raise the cue, 4 * NBUF + 3 = 19 dense
    let it lapse, two sparse raise it again, two dense follow with the list
    still on."""
    rng = np.random.default_rng(seed)
    z = W.ZipfSampler(300, 1.1)
    out, fresh = [], 5000
    for k, kind in enumerate("ss" + "d" * 19 + "ss" + "dd"):
        if kind == "s":
            t = z.sample(rng, sparse_rpb)
        else:  # half new tenants, half the previous dense batch's (live slots)
            t = rng.permutation(np.r_[fresh + np.arange(dense_tenants), fresh - np.arange(1, dense_tenants + 1)])
            fresh += dense_tenants
        out.append(W.c1_batch(t, NOW0 + k // 2, rng.integers(1, 9, t.size).astype(np.uint32)))
    return out


@functools.lru_cache(maxsize=None)
def _cue(lc):
    bs = _cue_batches(1500, 3000, 31)
    return bs, _oracle(bs, lc)


@functools.lru_cache(maxsize=None)
def _cue_collide(lc):
    """The same on 13 hash bits: a dense batch's 1200 stems share 8192 sort
    keys, so it holds tens of runs of two unrelated stems (k_run_check unmarks
    both: keys seen once after all) beside a few of three (k_split)."""
    bs = _cue_batches(300, 600, 32)
    return bs, _oracle(bs, lc)


def _mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("RL_LIST_CUE", raising=False)
    else:
        monkeypatch.setenv("RL_LIST_CUE", mode)


@pytest.mark.parametrize("lc", [False, True])
@pytest.mark.parametrize("mode", CUE_MODES)
def test_gpu_list_cue_raised_lapsed_and_raised_again_vs_c_oracle(monkeypatch, mode, lc):
    _mode(monkeypatch, mode)
    bs, want = _cue(lc)
    _check(bs, want, lc)


@pytest.mark.parametrize("mode", CUE_MODES)
def test_gpu_list_cue_with_isolated_failures_vs_c_oracle(monkeypatch, mode):
    _mode(monkeypatch, mode)
    bs, want = _cue(False)
    _check(bs, want, False, isolate=True)


@pytest.mark.parametrize("lc", [False, True])
@pytest.mark.parametrize("mode", CUE_MODES)
def test_gpu_list_cue_with_colliding_sort_keys_vs_c_oracle(monkeypatch, mode, lc):
    _mode(monkeypatch, mode)
    bs, want = _cue_collide(lc)
    _check(bs, want, lc, debug_hash_bits=13)


@pytest.mark.parametrize("lc", [False, True])
@pytest.mark.parametrize("mode", CUE_MODES)
def test_gpu_big_bucket_runs_of_one_with_and_without_the_list(monkeypatch, mode, lc):
    """magnitude.s_big: a large bucket sorts every element, so its light keys
    are runs of one in the sorted order: listed by k_run_check with the list
    on, answered in arrival order without it."""
    _mode(monkeypatch, mode)
    want, _ = M.reference("big", "now0", lc)
    _check(M.stream("big", "now0"), want, lc, isolate=True, max_batch=1 << 15)
