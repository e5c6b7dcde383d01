"""The engine at the top of the u32 range: limits, addends and counts up to
2^32 - 1, clocks at 0 and at NOW_MAX.

Every other GPU test keeps limits, addends and counts below 2^15 and runs at
one clock; the counting arithmetic the kernels redo by hand (simple_step,
general_step, k_fast_over / fast_emit_body, the in-run prefix sums, the
big-bucket class sums, alias_setup, the history log, k_lookup, export / import,
the routed records) would hide a signed comparison, a sum in fewer bits, a
float conversion or a packed field there. Each test below takes the batch
shape of the existing test that reaches one of those paths and changes only
the values (magnitude.scale, magnitude.crossing_runs). The references are the
C oracle and, in exact integers, magnitude.ExactModel; tests/test_magnitude_cpu.py
proves on the same stream objects that they agree and that no count passes
2^32 - 1. Every case runs with per-descriptor statuses and requires them all
zero, and compares code, limit_remaining, reset_s and stats bit for bit."""
import numpy as np
import pytest

from oracle import oracle as O
from ratelimit_amd import abi, workloads as W
from ratelimit_amd.limiter import Backend, GpuRateLimitCache, migrate
import golden_util as G
import magnitude as M
import streams

pytestmark = pytest.mark.gpu

CTX = dict(table_slots=1 << 17, max_batch=1 << 15, max_rules=8)
EPOCHS = list(M.CLOCK_EPOCHS)


def _same(g, want, model, a, n, k, keep=None):
    """The engine's answers against the C oracle's and the model's (both over
    the descriptors of `keep` only, where given)."""
    if keep is None:
        assert not g["status"].any(), "batch %d: statuses %s" % (k, np.unique(g["status"]))
        got = g
    else:
        got = {f: g[f][keep] for f in ("code", "limit_remaining", "reset_s")}
        got["stats"] = g["stats"]
        a, n, _ = streams.drop_descriptors(a, n, 0, keep)
    for who, ref in (("C oracle", want), ("model", model)):
        if ref is None:
            continue
        for f in M.FIELDS:
            assert np.array_equal(got[f], ref[f]), M.explain(got, ref, model, a, n, "batch %d, engine vs %s:" % (k, who))


def _run(name, epoch, lc, **kw):
    bs = M.stream(name, epoch)
    want, model = M.reference(name, epoch, lc)
    be = Backend(0.8, lc, **{**CTX, **kw})
    try:
        for k, (a, n, nq, nr) in enumerate(bs):
            _same(be.do_limit_arrays(a, n, nq, nr, isolate=True), want[k], model[k], a, n, k)
    finally:
        be.close()
    M.coverage(name, bs, model, lc)


path = pytest.mark.parametrize("epoch", EPOCHS)
cache = pytest.mark.parametrize("lc", [False, True])


# --------------------------------------------------------------------------- the decide kernel
@pytest.mark.parametrize("ratio", [0.8, 1.0, 1.25])
def test_gpu_decide_grid_vs_python_decide(ratio):
    """rl_debug_decide on before x hits x limit x shadow x local-cache hit
    (magnitude.decide_grid), one call: code, remaining, the six stat deltas and
    the local-cache set against the Python oracle's GetResponseDescriptorStatus
    (at ratio 1.25 the near threshold wraps in u32, in both alike)."""
    grid = M.decide_grid()
    be = Backend(ratio, True, **CTX)
    try:
        n = len(grid)
        code, rem, _, deltas, lc_set = be.debug_decide(
            [c[0] for c in grid], [c[1] for c in grid], [c[2] for c in grid], [c[3] for c in grid],
            [c[4] for c in grid], [2] * n, [abi.RL_FLAG_SHADOW if c[5] else 0 for c in grid], [0] * n)
    finally:
        be.close()
    for i, c in enumerate(grid):
        want = M.python_decide(ratio, True, c)
        got = (int(code[i]), int(rem[i]), tuple(int(x) for x in deltas[i]), bool(lc_set[i]))
        assert got == want, (ratio, c, got, want)


# --------------------------------------------------------------------------- one test per engine path
@cache
@path
def test_gpu_keys_seen_once_vs_c_oracle_and_model(epoch, lc):
    """Path 1: keys seen once, answered in arrival order (magnitude.s_once)."""
    _run("once", epoch, lc)


@cache
@path
def test_gpu_short_runs_vs_c_oracle_and_model(epoch, lc):
    """Path 2: runs of 3..20 on replay_simple / simple_step (magnitude.s_short)."""
    _run("short", epoch, lc)


@cache
@path
def test_gpu_long_runs_vs_c_oracle_and_model(epoch, lc):
    """Path 3: RUN_FAST runs of 33..120 over 256-position blocks, the limit
    crossed at the first, a middle and the last element (magnitude.s_long)."""
    _run("long", epoch, lc)


@cache
@path
def test_gpu_colliding_sort_keys_vs_c_oracle_and_model(epoch, lc):
    """Path 4: k_split, 4k stems on 13 hash bits (magnitude.s_split)."""
    _run("split", epoch, lc, debug_hash_bits=13)


@pytest.mark.parametrize("mode", ["0", "2"])
@cache
@path
def test_gpu_split_long_runs_vs_c_oracle_and_model(monkeypatch, epoch, lc, mode):
    """Path 5: two sort keys for six stems, runs of thousands whose sum ends
    just under 2^32, walked by k_split's own workgroups (RL_SPLIT_LONG=0) and
    by k_split_long (2) (magnitude.s_split_long)."""
    monkeypatch.setenv("RL_SPLIT_LONG", mode)
    _run("split_long", epoch, lc, debug_hash_bits=1, hash_seed=11)


@cache
@path
def test_gpu_multi_unit_alias_path_vs_c_oracle_and_model(epoch, lc):
    """Path 6: hot stems under SECOND and MINUTE, limits of both from the edge
    set; at clock 0 the two units share one key (magnitude.s_alias)."""
    _run("alias", epoch, lc)


@cache
@path
def test_gpu_multi_unit_exact_path_vs_c_oracle_and_model(epoch, lc):
    """Path 7: the clock changes inside the batch, multi-unit stems take
    general_step (magnitude.s_exact)."""
    _run("exact", epoch, lc)


@cache
@path
def test_gpu_big_bucket_vs_c_oracle_and_model(epoch, lc):
    """Path 8: k_bucket queues a sort bucket (the top 10 key bits) for
    k_big_count / k_big_place / k_bucket_big once it holds more than
    BkSmall::CAP = 2048 descriptors (`S > B::CAP` in k_bucket). One tenant with
    magnitude.BIG_HOT = 2100 requests puts 2100 descriptors of one stem into one
    bucket, twice (its sec and its min stem); the first such batch runs the
    one-workgroup grids, the second the full ones (magnitude.s_big)."""
    assert M.BIG_HOT > 2048
    _run("big", epoch, lc)


@pytest.mark.parametrize("unit", ["second", "minute"])
@cache
@path
def test_gpu_history_returns_large_counts_vs_c_oracle_and_model(epoch, lc, unit):
    """Path 9: counts above 2^31 in window w, the key moved to w + 1, then back
    in w: the count comes back from the history log exactly, also for a run of
    60 on the older window (magnitude.s_history_*)."""
    _run("history_" + unit, epoch, lc)


# --------------------------------------------------------------------------- clock edges
@cache
def test_gpu_clock_zero_hour_and_day_units(lc):
    """Clock 0 and 59, HOUR and DAY: windowStart 0, reset 3600 - now / 86400 - now."""
    _run("zero_units", "now0", lc)
    a = M.stream("zero_units")[2][0]
    want = M.reference("zero_units", "now0", lc)[0][2]
    assert set(want["reset_s"][a["unit"] == 4].tolist()) == {86400 - 59}


@cache
def test_gpu_clock_top_of_the_range(lc):
    """A batch at NOW_MAX - 2, then one at exactly NOW_MAX (DAY) in which one
    request at NOW_MAX + 1 alone is RL_E_TIME, then rl_sweep(NOW_MAX) and one
    more batch at NOW_MAX: every other answer exact (magnitude.s_top)."""
    bs = M.stream("top")
    want, model = M.reference("top", "now0", lc)
    be = Backend(0.8, lc, **CTX)
    try:
        a, n, nq, nr = bs[0]
        _same(be.do_limit_arrays(a, n, nq, nr, isolate=True), want[0], model[0], a, n, 0)
        a, n, nq, nr = bs[1]
        keep = M.top_keep(bs[1])
        g = be.do_limit_arrays(a, n, nq, nr, isolate=True)
        assert (g["status"][~keep] == abi.RL_E_TIME).all() and not g["status"][keep].any(), np.unique(g["status"])
        _same(g, want[1], model[1], a, n, 1, keep=keep)
        assert be.sweep(M.NOW_MAX) > 0  # (the SECOND keys of NOW_MAX - 2 are dead)
        a, n, nq, nr = bs[2]
        _same(be.do_limit_arrays(a, n, nq, nr, isolate=True), want[2], model[2], a, n, 2)
    finally:
        be.close()
    M.coverage("top", bs, model, lc)


# --------------------------------------------------------------------------- known answers and call streams
@cache
def test_gpu_known_answers(lc):
    """tests/golden/own_u32_edges.json: hand-computed codes and remainders."""
    be = Backend(0.8, lc, **CTX)
    try:
        for k, (b, expect, names) in enumerate(M.golden_batches(M.golden_cases(), lc)):
            g = be.do_limit_arrays(*b, isolate=True)
            assert not g["status"].any()
            got = list(zip(g["code"].tolist(), g["limit_remaining"].tolist()))
            assert got == expect, (k, [(nm, x, e) for nm, x, e in zip(names, got, expect) if x != e])
    finally:
        be.close()


@pytest.mark.parametrize("where,seed", M.RANDOM_CASES)
def test_gpu_random_call_streams_vs_python_oracle(where, seed):
    """Structured call streams with limits around 2^31 and 2^32 - 128, every
    key primed to just below them (magnitude.primed_stream), through
    GpuRateLimitCache in uneven chunks against the Python oracle."""
    n_calls, limit_range, prime = M.RANDOM_RANGES[where]
    calls = M.primed_stream(seed, limit_range, prime, n_calls=n_calls, zipf=seed % 2 == 0, **M.RANDOM_KW)
    lc = bool(seed % 2)
    py_out, py_stats = streams.python_oracle_run(calls, 0.8, lc, "", False)
    exp = [[s.as_tuple() for s in o] for o in py_out]
    streams.reset_stats(calls)
    cache_ = GpuRateLimitCache(None, 0.8, lc, "", False, table_slots=1 << 16, max_batch=1 << 14, max_rules=1 << 10)
    outs = []
    try:
        i, step = 0, 1
        while i < len(calls):
            outs += cache_.do_limit_batch(calls[i:i + step])
            i += step
            step = step % 7 + 2
    finally:
        cache_.close()
    got = [[G.status_tuple(s) for s in o] for o in outs]
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, "call %d: gpu %s oracle %s" % (i, g, e)
    stats = {l.stats.key: l.stats.as_tuple() for _, ls, _ in calls for l in ls if l is not None}
    assert stats == py_stats


# --------------------------------------------------------------------------- downstream of the counters
@pytest.mark.parametrize("epoch", ["zero", "top"])
def test_gpu_lookup_reads_counts_at_the_top(epoch):
    """Backend.lookup of keys counted to 2^31 - 1, 2^31 and 2^32 - 1: count,
    expire and the local-cache entry as the model holds them."""
    (a, n, nq, nr), = M.stream("counted", epoch)
    now = M.CLOCK_EPOCHS[epoch]
    m = M.ExactModel(0.8, True)
    mo = m.do_limit(a, n, nq, nr)
    be = Backend(0.8, True, **CTX)
    try:
        _same(be.do_limit_arrays(a, n, nq, nr, isolate=True), None, mo, a, n, 0)
        stems = M.stems_of(a, n)
        res = be.lookup(stems, a["unit"], [now] * n)
        assert not res["status"].any() and res["found"].all()
        for i, s in enumerate(stems):
            d = M.DIV[int(a["unit"][i])]
            cnt, exp = m.redis[(s, now // d * d)]
            assert (int(res["count"][i]), int(res["expire"][i])) == (cnt, exp), (i, res["count"][i], cnt)
            assert int(res["lc"][i]) == m.lc.get((s, now // d * d), 0), i
        assert sorted(set(res["count"].tolist())) == [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
        assert int((res["lc"] != 0).sum()) == 2
    finally:
        be.close()


@pytest.mark.parametrize("how", ["migrate", "snapshot"])
@cache
def test_gpu_large_counts_survive_export_import_and_snapshot(lc, how):
    """Two batches on ctx A; export_records -> import_records into a ctx with
    another table_slots and hash_seed (or snapshot save / load into a twin);
    the third batch, which crosses limits from counts above 2^31, continues
    bit-exactly there."""
    bs = M.stream("once", "top")
    want, model = M.reference("once", "top", lc)
    a = Backend(0.8, lc, **CTX)
    b = Backend(0.8, lc, **(dict(table_slots=1 << 14, max_batch=1 << 15, max_rules=8, hash_seed=99)
                            if how == "migrate" else CTX))
    try:
        for k in (0, 1):
            x, n, nq, nr = bs[k]
            _same(a.do_limit_arrays(x, n, nq, nr, isolate=True), want[k], model[k], x, n, k)
        if how == "migrate":
            tot = migrate(a, b)
            assert tot["keys"] == a.table_info()["live_slots"] == b.table_info()["live_slots"] == 4000
            rec = np.concatenate([r["count"] for r in a.export_records()])
            assert int(rec.max()) > 2 ** 31
        else:
            b.load_snapshot(a.snapshot())
        x, n, nq, nr = bs[2]
        _same(b.do_limit_arrays(x, n, nq, nr, isolate=True), want[2], model[2], x, n, 2)
        codes = model[2]["code"]
        big = np.array([v is not None and v > 2 ** 31 for v in model[2]["before"]])
        assert (codes[big] == M.OK).any() and (codes[big] == M.OVER).any()
    finally:
        a.close()
        b.close()


@cache
def test_gpu_two_shards_route_wide_values(lc):
    """n_shards=2: the routed Wire record's limit and hits and pack_res's
    remaining carry all 32 bits (the short-run stream)."""
    _run("short", "now0", lc, n_shards=2, shard_devices=[0, 0], hash_seed=77, max_rules=16)


def test_gpu_loopback_world_2_routes_wide_values():
    """The library router at world 2 over the loopback transport."""
    from test_gpu_loopback import _check as lb_check, run_world
    cfg = (0.8, True, False)
    batches = M.stream("short", "now0")
    out = run_world(2, batches, cfg)
    for r in range(2):
        assert out[r][0] == "ok", out[r][1]
    lb_check(out, batches, cfg, 2)


# --------------------------------------------------------------------------- the device-tensor entry point
def _dev(a):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else
                                np.ascontiguousarray(v)).cuda() for k, v in a.items()}


def test_gpu_device_tensors_carry_values_above_2_pow_31():
    """do_limit_device: int32 tensors built with a numpy view hold the same bits
    as the uint32 arrays, and the answers (int32 tensors viewed back) equal the
    host path's references."""
    import torch
    bs = M.stream("once", "now0")
    want, model = M.reference("once", "now0", False)
    assert int(bs[2][0]["hits"].max()) == 2 ** 32 - 1 and int(bs[0][0]["limit"].max()) == 2 ** 32 - 1
    assert max(model[2]["after"]) == 2 ** 32 - 1
    be = Backend(0.8, False, **CTX)
    try:
        keep = []
        for a, n, nq, nr in bs:
            d = _dev(a)
            assert np.array_equal(d["hits"].cpu().numpy().view(np.uint32), a["hits"])
            o = {"code": torch.zeros(n, dtype=torch.uint8, device="cuda"),
                 "limit_remaining": torch.zeros(n, dtype=torch.int32, device="cuda"),
                 "reset_s": torch.zeros(n, dtype=torch.int32, device="cuda"),
                 "stats": torch.zeros(nr * abi.RL_NUM_STATS, dtype=torch.int64, device="cuda"),
                 "status": torch.zeros(n, dtype=torch.uint8, device="cuda")}
            torch.cuda.synchronize()
            be.do_limit_device(d, o, n, nq, nr)
            keep.append((d, o))
        be.synchronize()
        for k, ((a, n, nq, nr), (_, o)) in enumerate(zip(bs, keep)):
            g = {"code": o["code"].cpu().numpy(), "status": o["status"].cpu().numpy(),
                 "limit_remaining": o["limit_remaining"].cpu().numpy().view(np.uint32),
                 "reset_s": o["reset_s"].cpu().numpy().view(np.uint32),
                 "stats": o["stats"].cpu().numpy().view(np.uint64)}
            _same(g, want[k], model[k], a, n, k)
    finally:
        be.close()


def test_gpu_c1_batch_dev_keeps_wide_hits():
    """workloads.c1_batch_dev(hits=...) on the device: the int32 tensors hold the
    bits of c1_batch's uint32 arrays for addends up to 2^32 - 1."""
    t = np.arange(7)
    h = np.array(M.HITS_EDGES, np.uint32)
    a, n, nq, nr = W.c1_batch(t, M.NOW_MAX, h)
    for hits in (h, h.astype(np.int64).tolist()):
        d, dn, dq, dr = W.c1_batch_dev(t, M.NOW_MAX, hits)
        assert (dn, dq, dr) == (n, nq, nr)
        for k, v in a.items():
            got = d[k].cpu().numpy()
            assert np.array_equal(got.view(v.dtype) if got.dtype != v.dtype else got, v), k


# --------------------------------------------------------------------------- payloads in, payloads out
def _wide_config():
    import yaml
    rules = [("wide", "minute", 2 ** 32 - 1), ("sign", "hour", 2 ** 31), ("top2", "day", 2 ** 32 - 2),
             ("low", "second", 2 ** 24 + 1)]
    return [("mag.yaml", yaml.safe_dump({"domain": "mag", "descriptors": [
        {"key": k, "rate_limit": {"unit": u, "requests_per_unit": r}} for k, u, r in rules]}))]


def _wide_requests(n_pairs=120):
    """Pairs of requests on the keys (rule, v<pair>): the two addends of a pair
    (5-byte varints among them) sum to at most 2^32 - 1, so every count stays a
    u32; every sixth pair carries a per-request override whose requests_per_unit
    is from the top edges too."""
    pairs = [(2 ** 31, 2 ** 31 - 1), (2 ** 32 - 2, 1), (2 ** 31 - 1, 2 ** 31), (2 ** 31 + 1, 5), (2 ** 32 - 1, 0),
             (2 ** 16, 2 ** 31), (2 ** 24 + 1, 2 ** 32 - 2 ** 25)]
    sets = [("wide",), ("sign", "top2"), ("low", "wide", "sign"), ("top2",)]
    reqs, nows = [], []
    for p in range(n_pairs):
        for j, h in enumerate(pairs[p % len(pairs)]):
            if j == 1 and h == 0:
                continue  # (2^32 - 1 fills the key alone)
            descs = []
            for k in sets[p % len(sets)]:
                lim = None
                if p % 6 == 0 and k != "low":
                    lim = O.Limit([2 ** 31 - 1, 2 ** 32 - 2, 2 ** 31 + 1][p // 6 % 3], O.MINUTE if k == "wide" else O.DAY)
                descs.append(O.Descriptor([(k, "v%d" % p)], lim))
            reqs.append(O.RateLimitRequest("mag", descs, h))
            nows.append(1_700_000_040 + p // 40)
    return reqs, nows


@pytest.mark.parametrize("lc,global_shadow", [(False, False), (True, True)])
def test_gpu_wide_payloads_to_response_bytes_match_oracle_service(lc, global_shadow):
    """RateLimitRequest payloads whose hits_addend is a 5-byte varint, a config
    and per-request overrides whose requests_per_unit is from the top edges,
    through rl_do_limit_wire_respond_async
    (should_rate_limit_responses_pipelined): the response bytes equal
    tests/response_ref.py fed from the oracle service, as in
    test_gpu_respond_stream_matches_oracle_service: 10-digit header values
    and wide response varints end to end."""
    from oracle.config import OracleService, RateLimitConfig, StatsStore
    from ratelimit_amd.limiter import GpuRateLimitService
    import pbwire
    import response_ref as R
    import verdict_ref as V
    from test_gpu_requests import SMALL, st_tuple
    from test_gpu_respond import STD_KEYS, desc_of
    from test_gpu_wire import cuts_of
    files = _wide_config()
    reqs, nows = _wide_requests()
    msgs = [pbwire.encode_request(r) for r in reqs]
    assert sum(len(pbwire.varint(r.hits_addend)) == 5 for r in reqs) > 100
    cuts = cuts_of(3, len(reqs), sizes=(1, 7, 64))
    group = 4

    def deferred(q):  # a descriptor with a limit override
        return any(d.limit is not None for d in reqs[q].descriptors)

    order = []  # as the service applies them: per group the requests without an override, then the deferred ones
    for g in range(0, len(cuts), group):
        part = cuts[g:g + group]
        for i, j in part:
            order += [q for q in range(i, j) if not deferred(q)]
        for i, j in part:
            order += [q for q in range(i, j) if deferred(q)]
    assert sum(1 for q in order if deferred(q)) >= 20
    store = StatsStore()
    oc = O.OracleFixedRateLimitCache(0.8, lc, "")
    osvc = OracleService(RateLimitConfig(files, store), oc, global_shadow)
    want = {}
    for q in order:
        _, unl = osvc.construct_limits_to_check(reqs[q])
        ocode, osts, _ = osvc.should_rate_limit(reqs[q], nows[q])
        v = V.verdict(osts, unl, global_shadow)
        assert v.code == ocode
        want[q] = (v, [st_tuple(s) for s in osts], unl)
    added = {}
    for op, key, h in oc.client.log:  # (no count of the oracle's store passed 2^32 - 1)
        if op == "INCRBY":
            added[key] = added.get(key, 0) + h
    assert 2 ** 31 < max(added.values()) <= M.U32_MAX
    ostats = {k: list(v.as_tuple()) for k, v in store.by_key.items() if any(v.as_tuple())}
    svc = GpuRateLimitService(files, 0.8, lc, "", global_shadow_mode=global_shadow, header_keys=STD_KEYS, **SMALL)
    got, shadow = [], 0
    try:
        for g in range(0, len(cuts), group):
            batches = [(msgs[i:j], nows[i:j]) for i, j in cuts[g:g + group]]
            for part, n in svc.should_rate_limit_responses_pipelined(batches):
                got += part
                shadow += n
        assert svc.global_shadow_count == shadow and len(got) == len(reqs)
        wide_rem = over = 0
        for q, raw in enumerate(got):
            v, sts, unl = want[q]
            code, dsts, hdrs = R.decode_response(raw)
            assert code == v.code, q
            assert dsts == sts, (q, dsts, sts)
            hw = [] if v.headers is None else [(k, b"%d" % x) for k, x in zip(STD_KEYS, v.headers)]
            assert hdrs == hw, q
            descs = [desc_of(s, u) for s, u in zip(sts, unl)]
            assert raw == R.encode_response(v.code, descs, v.headers, STD_KEYS), q
            over += v.flags & 1
            wide_rem += any(s[2] >= 2 ** 31 for s in sts)
        assert over > 0 and wide_rem > 20
        assert any(len(v) == 10 for _, v in R.decode_response(got[0])[2])  # (a 10-digit header value)
        assert dict(svc.stats) == ostats
        assert shadow == sum(v.shadow_inc for v, _, _ in want.values())
    finally:
        svc.close()
