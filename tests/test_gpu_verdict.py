"""GPU parity of the per-request verdict (rl_do_limit_requests_verdict,
rl_debug_verdict): the overall code, the minimumDescriptor behind the
RateLimit-* headers and global shadow mode of shouldRateLimitWorker
(src/service/ratelimit.go:163-209) on the device, against the sequential
restatement (tests/verdict_ref.py):

* the reference's own service tests (tests/golden/ref_service_verdict.json);
* synthetic per-descriptor answers whose requests straddle the 64-lane and
  256-lane boundaries, with ties and first-only / last-only OVER_LIMIT;
* the C4 request streams of tests/test_gpu_requests.py end to end, with
  per-descriptor outputs, verdict-only, on a 2-shard ctx, and against the old
  entry point, whose outputs must not change.
"""
import ctypes as C
import functools
import json
import os
import random

import numpy as np
import pytest

import verdict_ref as V
from oracle import oracle as O
from oracle.config import OracleService, RateLimitConfig, StatsStore
from ratelimit_amd import abi
from ratelimit_amd.config import ConfigTree, pack_requests
from ratelimit_amd.limiter import Backend, GpuRateLimitService, RedisError
from ratelimit_amd.packing import RuleInterner
from test_gpu_requests import FILES, SMALL, gen_requests, st_tuple

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_service_verdict.json")))
NONE, UNLIMITED, LIMIT = abi.RL_MATCH_NONE, abi.RL_MATCH_UNLIMITED, abi.RL_MATCH_LIMIT
U32 = 0xFFFFFFFF
VERDICT_KEYS = tuple(abi.REQUEST_VERDICT_DTYPES)


def flatten(requests):
    """[[(match, Status)] per request] -> rl_debug_verdict's input arrays."""
    cols = {k: [] for k in ("req_idx", "match", "code", "rem", "reset", "rpu")}
    for q, descs in enumerate(requests):
        for m, s in descs:
            cols["req_idx"].append(q)
            cols["match"].append(m)
            cols["code"].append(s.code)
            cols["rem"].append(s.limit_remaining)
            cols["reset"].append(s.duration_until_reset or 0)
            cols["rpu"].append(s.current_limit.requests_per_unit if s.current_limit else 0)
    return cols


def expected_arrays(verdicts, firsts):
    """[V.Verdict] and each request's first batch index -> the rl_request_verdict arrays."""
    nq = len(verdicts)
    e = {k: np.zeros(nq, dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
    for q, (v, d0) in enumerate(zip(verdicts, firsts)):
        e["overall_code"][q] = v.code
        e["flags"][q] = v.flags
        e["min_descriptor"][q] = U32 if v.min_index is None else d0 + v.min_index
        if v.headers is not None:
            e["header_limit"][q], e["header_remaining"][q], e["header_reset_s"][q] = v.headers
    e["global_shadow"] = sum(v.shadow_inc for v in verdicts)
    return e


def check_debug_verdict(be, requests, global_shadow):
    cols = flatten(requests)
    got = be.debug_verdict(len(requests), cols["req_idx"], cols["match"], cols["code"], cols["rem"], cols["reset"],
                           cols["rpu"], global_shadow)
    firsts = np.concatenate([[0], np.cumsum([len(r) for r in requests])])[:-1]
    want = expected_arrays([V.verdict([s for _, s in r], [m == UNLIMITED for m, _ in r], global_shadow)
                            for r in requests], firsts)
    for k in VERDICT_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert got["global_shadow"] == want["global_shadow"]
    return got


@pytest.fixture(scope="module")
def backend():
    be = Backend(**SMALL)
    yield be
    be.close()


@pytest.mark.parametrize("global_shadow", [False, True])
def test_gpu_verdict_reference_service_tests(backend, global_shadow):
    """The reference's mocked-status vectors, each alone and all as one batch."""
    reqs = []
    for case in GOLDEN["cases"]:
        r = [(LIMIT if s.current_limit else NONE, s) for s in V.golden_statuses(case)]
        reqs.append(r)
        got = check_debug_verdict(backend, [r], global_shadow)
        if global_shadow == case["global_shadow_mode"]:
            exp = case["expect"]
            assert got["overall_code"][0] == exp["overall_code"]
            assert got["global_shadow"] == exp["global_shadow_mode_counter"]
            if case["headers_enabled"]:
                assert [str(int(got[k][0])) for k in ("header_limit", "header_remaining", "header_reset_s")] \
                    == exp["headers"]
    check_debug_verdict(backend, reqs, global_shadow)


def synthetic_descriptor(rng, over_p=0.1):
    x = rng.random()
    if x < 0.2:
        return NONE, V.Status(V.OK, None, 0, None)
    if x < 0.35:
        return UNLIMITED, V.Status(V.OK, None, U32, None)
    lim = V.Limit(rng.randint(0, 1000), rng.randint(1, 4))
    if rng.random() < over_p:
        return LIMIT, V.Status(V.OVER_LIMIT, lim, 0, rng.randint(1, 86400))
    return LIMIT, V.Status(V.OK, lim, rng.choice([0, 1, 2, 3, U32 - 1]), rng.randint(1, 86400))


def synthetic_batch():
    """~3,400 descriptors; request sizes put segments on both sides of the 64-lane
    and 256-lane boundaries: e.g. request 1 ends at lane 63 exactly, the 700 of
    the first round starts at 707 and covers three whole workgroups' tails and
    heads, the 256 after it starts at 1407 (lane 63 of a wave)."""
    rng = random.Random(20260)
    sizes = [1, 63, 2, 64, 0, 65, 255, 257, 700, 256] + [700, 0, 257, 1, 256, 65, 2, 255, 64, 63]
    reqs = [[synthetic_descriptor(rng) for _ in range(n)] for n in sizes]

    def only_over(n, where):
        ok = lambda: V.Status(V.OK, V.Limit(50, 2), rng.choice([0, 1, 2, 3]), rng.randint(1, 60))  # noqa: E731
        r = [(LIMIT, ok()) for _ in range(n)]
        r[where] = (LIMIT, V.Status(V.OVER_LIMIT, V.Limit(7, 1), 0, 1))
        return r

    # only the first / only the last descriptor OVER_LIMIT, in requests that span waves and workgroups
    reqs[5] = only_over(65, 0)
    reqs[7] = only_over(257, -1)
    reqs[10] = only_over(700, 0)
    reqs[12] = only_over(257, 0)
    reqs[15] = only_over(65, -1)
    reqs[17] = only_over(255, -1)
    assert [len(r) for r in reqs] == sizes and 3000 <= sum(sizes) <= 3500
    return reqs


@pytest.mark.parametrize("global_shadow", [False, True])
def test_gpu_verdict_synthetic_shapes(backend, global_shadow):
    got = check_debug_verdict(backend, synthetic_batch(), global_shadow)
    assert (got["global_shadow"] > 0) == global_shadow
    rng = random.Random(7)
    check_debug_verdict(backend, [[synthetic_descriptor(rng) for _ in range(300)]], global_shadow)  # one request only
    check_debug_verdict(backend, [[synthetic_descriptor(rng, 0.0) for _ in range(300)]], global_shadow)
    # a limited descriptor with MaxUint32 remaining is not below the loop's starting minimum (:166, :173)
    top = (LIMIT, V.Status(V.OK, V.Limit(U32, 2), U32, 9))
    check_debug_verdict(backend, [[top], [top, (LIMIT, V.Status(V.OK, V.Limit(5, 2), U32 - 1, 9))], []], global_shadow)


# ---- end to end ------------------------------------------------------------------

STREAMS = {1: dict(local_cache=False, global_shadow=False), 2: dict(local_cache=True, global_shadow=True)}


@functools.lru_cache(maxsize=None)
def oracle_stream(seed):
    """The oracle service's answers to gen_requests(seed, 1200) and the restatement's
    verdicts: computed once per seed, read-only afterwards."""
    p = STREAMS[seed]
    reqs, nows = gen_requests(seed, 1200)
    store = StatsStore()
    osvc = OracleService(RateLimitConfig(FILES, store), O.OracleFixedRateLimitCache(0.8, p["local_cache"], ""),
                         p["global_shadow"])
    verdicts, statuses = [], []
    for r, now in zip(reqs, nows):
        _, unl = osvc.construct_limits_to_check(r)
        ocode, osts, _ = osvc.should_rate_limit(r, now)
        v = V.verdict(osts, unl, p["global_shadow"])
        assert v.code == ocode
        verdicts.append(v)
        statuses.append(tuple(st_tuple(s) for s in osts))
    stats = {k: list(v.as_tuple()) for k, v in store.by_key.items() if any(v.as_tuple())}
    # the stream must exercise the order dependence (seeds 1 / 2 give 89 / 95, 34 / 47, 341 / 360, 237 / 252)
    n_over2 = n_tie = n_nolimit = n_notfirst = 0
    for v, sts in zip(verdicts, statuses):
        limited = [s for s in sts if s[1] is not None]
        n_over = sum(1 for s in limited if s[0] == V.OVER_LIMIT)
        n_over2 += n_over >= 2
        if not n_over and limited:
            lo = min(s[2] for s in limited)
            n_tie += lo < U32 and sum(1 for s in limited if s[2] == lo) >= 2
        n_nolimit += not limited
        n_notfirst += v.min_index is not None and v.min_index > 0
    assert n_over2 >= 50 and n_tie >= 20 and n_nolimit >= 100 and n_notfirst >= 100, \
        (n_over2, n_tie, n_nolimit, n_notfirst)
    return tuple(reqs), tuple(nows), tuple(verdicts), tuple(statuses), stats


def run_stream(seed, per_descriptor, **backend_kw):
    """The stream through should_rate_limit_verdicts in test_gpu_requests' random
    slices -> ([RequestVerdict], accumulated stats, accumulated global-shadow count)."""
    p = STREAMS[seed]
    reqs, nows = oracle_stream(seed)[:2]
    svc = GpuRateLimitService(FILES, 0.8, p["local_cache"], "", global_shadow_mode=p["global_shadow"],
                              **SMALL, **backend_kw)
    rng = random.Random(seed * 7)
    got, shadow = [], 0
    try:
        i = 0
        while i < len(reqs):
            j = min(len(reqs), i + rng.choice([1, 7, 64, 300]))
            part, n = svc.should_rate_limit_verdicts(reqs[i:j], nows[i:j], per_descriptor)
            got += part
            shadow += n
            i = j
        assert svc.global_shadow_count == shadow
        return got, dict(svc.stats), shadow
    finally:
        svc.close()


@functools.lru_cache(maxsize=None)
def gpu_stream(seed):
    return run_stream(seed, True)


def check_against_oracle(seed, got, stats, shadow, per_descriptor=True):
    _, _, verdicts, statuses, ostats = oracle_stream(seed)
    assert len(got) == len(verdicts)
    for g, v, sts in zip(got, verdicts, statuses):
        assert (g.code, g.flags, g.headers) == (v.code, v.flags, v.headers)
        if per_descriptor:
            assert tuple(st_tuple(s) for s in g.statuses) == sts
        else:
            assert g.statuses is None
    assert stats == ostats
    assert shadow == sum(v.shadow_inc for v in verdicts)
    assert (shadow > 0) == STREAMS[seed]["global_shadow"]


@pytest.mark.parametrize("seed", [1, 2])
def test_gpu_verdict_stream_matches_oracle_service(seed):
    check_against_oracle(seed, *gpu_stream(seed))


@pytest.mark.parametrize("seed", [1, 2])
def test_gpu_verdict_only_stream_equals_the_full_run(seed):
    """per_descriptor=False: no per-descriptor array crosses PCIe; the verdicts and
    the accumulated stats equal the run with them."""
    full, full_stats, full_shadow = gpu_stream(seed)
    got, stats, shadow = run_stream(seed, False)
    assert [(g.code, g.flags, g.headers) for g in got] == [(g.code, g.flags, g.headers) for g in full]
    assert stats == full_stats and shadow == full_shadow
    check_against_oracle(seed, got, stats, shadow, per_descriptor=False)


def test_gpu_verdict_multishard_stream_matches_oracle_service():
    check_against_oracle(2, *run_stream(2, True, n_shards=2, shard_devices=[0, 0], hash_seed=5))


def test_gpu_verdict_leaves_the_old_entry_point_unchanged():
    """The same batches through rl_do_limit_requests and rl_do_limit_requests_verdict
    on fresh ctxs: every per-descriptor array and the stats bytewise equal; with
    out == NULL (a third ctx) the verdict arrays equal those with outputs."""
    reqs, nows = gen_requests(2, 600)
    it = RuleInterner()
    tree = ConfigTree.from_yaml(FILES, "", it)
    bes = [Backend(0.8, True, **SMALL) for _ in range(3)]
    rng = random.Random(14)
    try:
        for be in bes:
            be.load_config(tree)
        i = 0
        while i < len(reqs):
            j = min(len(reqs), i + rng.choice([1, 7, 64, 300]))
            a = pack_requests(reqs[i:j], nows[i:j], it)
            n_rules = len(it.keys)
            old = bes[0].do_limit_requests(a, n_rules)
            new = bes[1].do_limit_requests_verdict(a, n_rules, global_shadow=True)
            only = bes[2].do_limit_requests_verdict(a, n_rules, global_shadow=True, per_descriptor=False, stats=False)
            assert set(old) == set(abi.REQUEST_RESULT_DTYPES) | {"stats"}
            for k in old:
                assert old[k].dtype == new[k].dtype and old[k].tobytes() == new[k].tobytes(), k
            assert set(only) == set(VERDICT_KEYS) | {"global_shadow"}
            for k in only:
                assert np.array_equal(only[k], new[k]), k
            i = j
    finally:
        for be in bes:
            be.close()


def test_gpu_verdict_errors():
    be = Backend(**SMALL)
    try:
        it = RuleInterner()
        be.load_config(ConfigTree.from_yaml(FILES, "", it))
        req = O.RateLimitRequest("c4", [O.Descriptor([("remote_address", "1")]),
                                        O.Descriptor([("remote_address", "50.0.0.5")])], 1)
        now = [1_700_000_000]

        def call(a, verdict, nq=1):
            b = abi.RlRequestBatch()
            b.n_requests, b.n_descriptors, b.n_entries, b.n_rules = nq, len(a["req_idx"]), len(a["key_len"]), \
                len(it.keys)
            for k in abi.REQUEST_ARRAYS:
                setattr(b, k, abi.ptr(a[k]))
            return be.L.rl_do_limit_requests_verdict(be.ctx, C.byref(b), None, 0,
                                                     None if verdict is None else C.byref(verdict))

        def verdict_struct(arrays, gs):
            v = abi.RlRequestVerdict()
            for k, x in arrays.items():
                setattr(v, k, abi.ptr(x))
            v.global_shadow = abi.ptr(gs)
            return v

        a = pack_requests([req], now, it)
        assert call(a, None) == abi.RL_E_INVALID
        arrays = {k: np.zeros(4, dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
        gs = np.zeros(1, np.uint64)
        for x in list(arrays.values()) + [gs]:
            x.view(np.uint8)[:] = 0xAB
        v = verdict_struct(arrays, gs)
        v.overall_code = None
        assert call(a, v) == abi.RL_E_INVALID
        # a malformed batch (request index out of range) leaves the verdict arrays alone
        bad = dict(a)
        bad["req_idx"] = a["req_idx"] + 5
        assert call(bad, verdict_struct(arrays, gs)) == abi.RL_E_INVALID
        for k, x in arrays.items():
            assert (x.view(np.uint8) == 0xAB).all(), k
        assert (gs.view(np.uint8) == 0xAB).all()
        # the good batch: 50.0.0.5 allows 0 per second, so the second descriptor is OVER_LIMIT
        assert call(a, verdict_struct(arrays, gs)) == abi.RL_OK
        assert (arrays["overall_code"][0], arrays["flags"][0], arrays["min_descriptor"][0]) == (V.OVER_LIMIT, 1, 1)
        assert (arrays["header_limit"][0], arrays["header_remaining"][0], arrays["header_reset_s"][0]) == (0, 0, 1)
        assert gs[0] == 0 and arrays["overall_code"][1] == 0xAB
        # rl_debug_verdict: a decreasing req_idx, or one beyond n_requests
        z = [0, 0]
        with pytest.raises(RedisError, match="RL_E_INVALID"):
            be.debug_verdict(2, [1, 0], z, z, z, z, z)
        with pytest.raises(RedisError, match="RL_E_INVALID"):
            be.debug_verdict(1, [0, 1], z, z, z, z, z)
        # no requests
        empty = be.debug_verdict(0, [], [], [], [], [], [])
        assert empty["global_shadow"] == 0 and len(empty["overall_code"]) == 0
        empty = be.do_limit_requests_verdict(pack_requests([], [], it), len(it.keys))
        assert empty["global_shadow"] == 0 and len(empty["overall_code"]) == 0
    finally:
        be.close()
