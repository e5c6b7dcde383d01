"""rl_lookup on the GPU: a key's counter, TTL and local-cache entry read without
counting a hit (Redis GET + TTL; Backend.lookup, GpuRateLimitCache.peek).

The answers are checked against the oracles' key stores, against what the
next request for the same key then reads, and against the batch path's own
RL_E_TIME verdicts; the call must leave every observable of the table as it
was.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle
from oracle import oracle as O
from ratelimit_amd import abi, workloads as W
from ratelimit_amd.limiter import Backend, FixedTimeSource, GpuRateLimitCache, KeyState, RedisError
from ratelimit_amd.packing import arrays_from_lists, stem_of
import streams
from test_gpu_history import _stream
from test_gpu_migrate import A_KW, _alias_expire_stream, _check, _export_all, _second_batch
from test_gpu_observability import stream as obs_stream

pytestmark = pytest.mark.gpu

OK, OVER = 1, 2  # RL_CODE_OK / RL_CODE_OVER_LIMIT
DIV = {1: 1, 2: 60, 3: 3600, 4: 86400}


def _all_ok(res):
    assert (res["status"] == abi.RL_OK).all(), np.unique(res["status"])


# --------------------------------------------------------------------------- 1. the oracle's stores
@pytest.mark.parametrize("per_second", [False, True])
def test_gpu_lookup_reads_the_oracles_stores(per_second):
    """Every (stem, unit) of the stream at the last clock T, one second and 61 s
    later: GET / TTL as the oracle's Redis store(s) hold the key, the local-cache
    entry as its freecache does."""
    calls = obs_stream(7)
    oc = O.OracleFixedRateLimitCache(0.8, True, per_second=per_second)
    for r, l, now in calls:
        oc.do_limit(r, l, now)
    T = calls[-1][2]
    keys = sorted({(stem_of("", r.domain, d.entries), lim.limit.unit)
                   for r, l, _ in calls for d, lim in zip(r.descriptors, l) if lim is not None})
    cache = GpuRateLimitCache(FixedTimeSource(0), 0.8, True, per_second=per_second, table_slots=1 << 16,
                              max_batch=1 << 14, max_rules=1 << 10)
    try:
        for i in range(0, len(calls), 500):
            cache.do_limit_batch(calls[i:i + 500])
        n_live = n_lc = 0
        for now in (T, T + 1, T + 61):
            res = cache.backend.lookup([k[0] for k in keys], [k[1] for k in keys], [now] * len(keys))
            _all_ok(res)
            for j, (stem, unit) in enumerate(keys):
                key = stem.decode() + str(now // DIV[unit] * DIV[unit])
                store = oc.per_second_client if per_second and unit == O.SECOND else oc.client
                e = store.data.get(key)  # (read without mutation: _live would delete a dead key)
                live = e is not None and (e[1] < 0 or now <= e[1])
                got = (int(res["found"][j]), int(res["count"][j]), int(res["expire"][j]))
                assert got == ((1, e[0], e[1]) if live else (0, 0, 0)), (key, now, got, e)
                lc = oc.local_cache.data.get(key, 0)
                assert int(res["lc"][j]) == (lc if lc > now else 0), (key, now)
                if now == T:
                    n_live += live
                    n_lc += lc > now
        assert n_live >= 40 and n_lc >= 10  # (what keeps this test honest)
    finally:
        cache.close()


# --------------------------------------------------------------------------- 2. peek, then hit
@pytest.mark.parametrize("seed,lc", [(21, False), (22, True)])
def test_gpu_lookup_then_hit_is_consistent(seed, lc):
    """Before each batch, the first descriptor of every distinct stem is looked
    up at its own unit and clock; the batch then answers it from that count.
    The C oracle replays the stream: its before = limit - remaining - hits
    where it answers OK; where it answers OVER_LIMIT without a local-cache hit
    the count read must put it over."""
    batches = _stream(seed, 2_000, 3_000, 8, 3, 7, multi=True, hot=200)
    be = Backend(0.8, lc, **A_KW)
    co = c_oracle.COracle(0.8, lc)
    try:
        seen = {"found": 0, "absent": 0, "lc": 0, "ok": 0, "over": 0}
        for i, (x, n, nq, nr) in enumerate(batches):
            L = int(x["stem_off"][1])
            _, first = np.unique(x["stem_bytes"].reshape(n, L), axis=0, return_index=True)
            first.sort()
            flat = x["stem_bytes"].reshape(n, L)
            res = be.lookup([flat[j].tobytes() for j in first], x["unit"][first], x["now"][x["req_idx"][first]])
            _all_ok(res)
            g, o = be.do_limit_arrays(x, n, nq, nr, isolate=True), co.do_limit(x, n, nq, nr)
            _check(g, o, i)
            h = np.maximum(x["hits"][first], 1).astype(np.int64)
            lim, cnt = x["limit"][first].astype(np.int64), res["count"].astype(np.int64)
            code, rem = o["code"][first], o["limit_remaining"][first].astype(np.int64)
            assert not x["flags"].any()  # (no shadow rules: a local-cache hit is OVER_LIMIT)
            if not lc:
                assert not res["lc"].any()
            hit = res["lc"] != 0
            assert (g["code"][first][hit] == OVER).all()
            assert (res["count"][res["found"] == 0] == 0).all()
            ok = ~hit & (code == OK)
            assert np.array_equal(cnt[ok], (lim - rem - h)[ok]), i
            over = ~hit & (code == OVER)
            assert (cnt[over] + h[over] > lim[over]).all(), i
            assert (ok | over | hit).all()
            seen["found"] += int(res["found"].sum())
            seen["absent"] += int((res["found"] == 0).sum())
            seen["lc"] += int(hit.sum())
            seen["ok"] += int(ok.sum())
            seen["over"] += int(over.sum())
        assert seen["found"] > 100 and seen["absent"] > 100 and seen["ok"] > 100 and seen["over"] + seen["lc"] > 0, seen
        assert (seen["lc"] > 0) == lc, seen
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 3. aliases by hand
M0 = W.NOW0 // 60 * 60 + 60
HAND = b"hand_built_stem_"


def _import(be, stem, recs):
    """recs: [(unit, flags, ws, count, expire, lc)] of one stem."""
    n = len(recs)
    cols = list(zip(*recs))
    be.import_records({
        "stem_bytes": np.frombuffer(stem * n, np.uint8).copy(), "stem_off": (len(stem) * np.arange(n + 1)).astype(np.uint32),
        "unit": np.array(cols[0], np.uint8), "flags": np.array(cols[1], np.uint8), "ws": np.array(cols[2], np.uint32),
        "count": np.array(cols[3], np.uint32), "expire": np.array(cols[4], np.uint32), "lc": np.array(cols[5], np.uint32)})


def _one(be, stem, unit, now):
    res = be.lookup([stem], [unit], [now])
    return tuple(int(res[k][0]) for k in ("status", "found", "count", "expire", "lc"))


@pytest.mark.parametrize("per_second", [False, True])
def test_gpu_lookup_alias_records_by_hand(per_second):
    """One stem under SECOND and MINUTE; at the minute's first second both units
    name one Redis key. The hand-built records differ (7 under SECOND, 5 under
    MINUTE), which shows whose is read: the first in unit order that is live
    and in the key's store."""
    be = Backend(0.8, True, per_second=per_second, table_slots=1 << 10, max_batch=64, max_rules=8, jitter=600)
    try:
        _import(be, HAND, [(1, 0, M0, 7, M0 + 1, M0 + 1), (2, 0, M0, 5, M0 + 60, 0)])
        assert be.table_info()["exact_stems"] == 2
        if not per_second:
            # one key: SECOND's record while it lives, its local-cache entry for both
            assert _one(be, HAND, 1, M0) == (0, 1, 7, M0 + 1, M0 + 1)
            assert _one(be, HAND, 2, M0) == (0, 1, 7, M0 + 1, M0 + 1)
            # one second later the keys differ: stem‖(M0 + 1) does not exist, stem‖M0 does
            assert _one(be, HAND, 1, M0 + 1) == (0, 0, 0, 0, 0)
            assert _one(be, HAND, 2, M0 + 1) == (0, 1, 7, M0 + 1, 0)
        else:
            # SECOND keys live in the per-second store: two keys, one local cache
            assert _one(be, HAND, 1, M0) == (0, 1, 7, M0 + 1, M0 + 1)
            assert _one(be, HAND, 2, M0) == (0, 1, 5, M0 + 60, M0 + 1)
            assert _one(be, HAND, 1, M0 + 1) == (0, 0, 0, 0, 0)
            assert _one(be, HAND, 2, M0 + 1) == (0, 1, 5, M0 + 60, 0)
        # the SECOND record dead: the MINUTE slot's own
        assert _one(be, HAND, 2, M0 + 2) == (0, 1, 5, M0 + 60, 0)
        assert _one(be, HAND, 2, M0 + 61) == (0, 0, 0, 0, 0)
        # a unit the stem has no slot of: its key (the hour's first second) is nobody's window here
        assert _one(be, HAND, 3, M0) == (0, 0, 0, 0, 0)
    finally:
        be.close()


def test_gpu_lookup_sees_an_expire_shortened_through_another_unit():
    """_alias_expire_stream: the MINUTE key of minute m, counted at m + 5, gets
    EXPIRE 1 from the SECOND request at m (the same Redis key): it is gone after
    m + 1, where ws + div would say live until m + 60."""
    bs = _alias_expire_stream(8)
    m = int(bs[1][0]["now"][0])
    stems = [b"alias_expire_stem_%03d_" % j for j in range(8)]
    be = Backend(0.8, True, table_slots=1 << 10, max_batch=64, max_rules=8)
    co = c_oracle.COracle(0.8, True)
    try:
        for i, bt in enumerate(bs[:2]):
            _check(be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt), i)
        res = be.lookup(stems, [2] * 8, [m + 1] * 8)
        _all_ok(res)
        assert res["found"].all() and (res["count"] == 2).all() and (res["expire"] == m + 1).all()
        res = be.lookup(stems + stems, [2] * 8 + [1] * 8, [m + 10] * 16)
        _all_ok(res)
        assert not res["found"].any() and not res["count"].any() and not res["expire"].any()
        _check(be.do_limit_arrays(*bs[2], isolate=True), co.do_limit(*bs[2]), 2)  # (the request agrees: count 1 again)
        res = be.lookup(stems, [2] * 8, [m + 10] * 8)
        assert res["found"].all() and (res["count"] == 1).all() and (res["expire"] == m + 70).all()
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 4. RL_E_TIME is mirrored
def _ask(be, stem, unit, now, limit=10):
    a = arrays_from_lists([stem], [now], [0], [unit], [0], [limit], [1], [0])
    return be.do_limit_arrays(a, 1, 1, 1, isolate=True)


@pytest.mark.parametrize("flag", [abi.RL_REC_CHAIN_LOST, 0])
def test_gpu_lookup_chain_lost_flag_by_hand(flag):
    """The window below a record flagged RL_REC_CHAIN_LOST may have had a
    record: RL_E_TIME from the lookup as from the request; without the flag it
    never had one (count 0)."""
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=64, max_rules=8, jitter=600)
    try:
        _import(be, HAND, [(1, flag, M0 + 10, 2, M0 + 11, 0), (1, 0, M0 + 13, 1, M0 + 14, 0), (2, 0, M0, 5, M0 + 90, 0)])
        got = _one(be, HAND, 1, M0 + 9)
        g = _ask(be, HAND, 1, M0 + 9)
        if flag:
            assert got == (abi.RL_E_TIME, 0, 0, 0, 0) and g["status"][0] == abi.RL_E_TIME
        else:
            assert got == (0, 0, 0, 0, 0) and g["status"][0] == 0 and g["limit_remaining"][0] == 9
        assert _one(be, HAND, 1, M0 + 10) == (0, 1, 2, M0 + 11, 0)  # the record itself, on the chain
        assert _one(be, HAND, 1, M0 + 13) == (0, 1, 1, M0 + 14, 0)  # cur
        assert _one(be, HAND, 1, M0 + 14) == (0, 0, 0, 0, 0)  # above cur: absent
        assert _one(be, HAND, 2, M0 + 30) == (0, 1, 5, M0 + 90, 0)  # the SECOND slot's lost record of M0 is dead by now
    finally:
        be.close()


WINDOWS, KEYS = 120, 1000


def test_gpu_lookup_time_errors_mirror_the_batch_path():
    """The smallest log under J = 600, wrapped by 1000 SECOND keys rolled through
    120 windows: every lookup of an older window is oracle-exact or RL_E_TIME, and
    the request batch for the same keys and clocks fails exactly those."""
    kw = dict(table_slots=1 << 16, max_batch=1 << 11, max_rules=8, jitter=600)
    be = Backend(0.8, True, history_entries=1, **kw)
    co = c_oracle.COracle(0.8, True, horizon=600)
    try:
        for k in range(WINDOWS):
            bt = _second_batch(KEYS, W.NOW0 + k)
            _check(be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt), k)
        info = be.table_info()
        assert info["history_appended"] > info["history_entries"]
        failed_total = ok_total = 0
        for back in (1, 3, 8, 20, 60, WINDOWS - 1):
            now = W.NOW0 + WINDOWS - 1 - back
            x, n, nq, nr = _second_batch(KEYS, now)
            L = int(x["stem_off"][1])
            res = be.lookup([r.tobytes() for r in x["stem_bytes"].reshape(n, L)], x["unit"], [now] * n)
            g = be.do_limit_arrays(x, n, nq, nr, isolate=True)
            failed = g["status"] != 0
            assert (g["status"][failed] == abi.RL_E_TIME).all(), np.unique(g["status"])
            print("back %d: lookup RL_E_TIME %d, batch RL_E_TIME %d, differing %d" % (
                back, int((res["status"] == abi.RL_E_TIME).sum()), int(failed.sum()),
                int(((res["status"] == abi.RL_E_TIME) != failed).sum())))
            assert np.array_equal(res["status"], np.where(failed, abi.RL_E_TIME, 0)), back
            o = co.do_limit(*streams.drop_descriptors(x, n, nq, ~failed), nr)
            for f in ("code", "limit_remaining", "reset_s"):
                assert np.array_equal(g[f][~failed], o[f]), (back, f)
            assert (o["code"] == OK).all()
            before = x["limit"][~failed].astype(np.int64) - o["limit_remaining"] - 1
            assert np.array_equal(res["count"][~failed], before), back
            assert np.array_equal(res["found"][~failed], before > 0), back  # (J = 0 draws: live until ws + 1 >= now)
            assert not res["count"][failed].any() and not res["found"][failed].any()
            failed_total += int(failed.sum())
            ok_total += int((~failed).sum())
        assert failed_total > 0 and ok_total > 0
        # below the sweep floor: RL_E_TIME, at it: answered
        T = W.NOW0 + WINDOWS
        be.sweep(T)
        stem = x["stem_bytes"][:L].tobytes()
        assert _one(be, stem, 1, T - 1)[0] == abi.RL_E_TIME and _ask(be, stem, 1, T - 1)["status"][0] == abi.RL_E_TIME
        assert _one(be, stem, 1, T)[0] == abi.RL_OK
        for bad in (-1, 0xFFFFFFFF - 2 * 86400 + 1, 1 << 40):  # clocks out of range
            assert _one(be, stem, 1, bad) == (abi.RL_E_TIME, 0, 0, 0, 0)
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 5. read-only
EVERY_LEN = list(range(1, 81)) + [255, 4096, 65535]


def _len_stems():
    return [(b"%05d/" % L * (L // 6 + 1))[:L] for L in EVERY_LEN]


def test_gpu_lookup_changes_nothing():
    """A table with history, tombstones and long stems: table_info, the
    local-cache gauges and the full export are the same before and after a
    lookup of present keys, never-seen stems and stems of every length."""
    be = Backend(0.8, True, table_slots=1 << 14, max_batch=1 << 12, max_rules=8, jitter=300)
    try:
        stream = _stream(6, 700, 1_000, 5, 20, 150)
        for x, n, nq, nr in stream:
            be.do_limit_arrays(x, n, nq, nr, isolate=True)
        T = W.NOW0 + 4 * 20 + 20
        ls = _len_stems()
        nl = len(ls)
        hits = [1 + j % 5 for j in range(nl)]
        a = arrays_from_lists(ls, [T] * nl, list(range(nl)), [2] * nl, [0] * nl, [1000] * nl, hits, [1] * nl)
        g = be.do_limit_arrays(a, nl, nl, 2, isolate=True)
        assert (g["status"] == 0).all()
        TS = W.NOW0 + 85  # the sweep's clock (the floor): every SECOND key of the stream is dead by then
        assert be.sweep(TS) > 0

        def readings():
            return be.table_info(), be.local_cache_info(T), sorted(_export_all(be)[0])

        r0 = readings()
        assert r0[0]["tombstones"] > 0 and r0[0]["history_slots"] > 0 and r0[0]["arena_bytes_used"] > 65535 - 32
        x, n, nq, nr = stream[-1]
        L = int(x["stem_off"][1])
        present = [r.tobytes() for r in x["stem_bytes"].reshape(n, L)]
        p_now = [int(t) for t in np.maximum(x["now"][x["req_idx"]], TS)]
        never = [b"never_seen_stem_%04d_" % j for j in range(1000)] + [s[:-1] + b"~" for s in ls]
        stems = present + never + ls
        units = [int(u) for u in x["unit"]] + [1 + j % 4 for j in range(len(never))] + [2] * nl
        nows = p_now + [T] * (len(never) + nl)
        res = be.lookup(stems, units, nows)
        _all_ok(res)
        r1 = readings()
        assert r0[0] == r1[0], "table_info changed"
        assert r0[1] == r1[1], "local-cache gauges changed"
        assert r0[2] == r1[2], "the export changed"
        for k in ("live_slots", "arena_bytes_used", "history_appended", "history_lost", "exact_stems"):
            assert r0[0][k] == r1[0][k], k
        lo, hi = len(present), len(present) + len(never)
        assert not res["found"][lo:hi].any() and not res["count"][lo:hi].any()
        assert res["found"][hi:].all() and list(res["count"][hi:]) == hits  # every length, inline and arena
        assert (res["expire"][hi:] == T + 60).all()
        # the present keys: the last batch's MINUTE keys of the floor's minute are live, with counts
        pm = np.array(units[:lo]) == 2
        assert res["found"][:lo][pm].any() and (res["count"][:lo][res["found"][:lo] == 1] > 0).all()
    finally:
        be.close()


# --------------------------------------------------------------------------- 6. probe paths
def _crowd(shards):
    """Hundreds of stems in a few home regions of a 2^10-slot table, a third of
    them swept away: tombstones lie on the probe paths of the rest."""
    kw = dict(table_slots=1 << 10, max_batch=1 << 10, max_rules=8, debug_hash_bits=2, hash_seed=9)
    if shards > 1:
        kw.update(n_shards=shards, shard_devices=[0] * shards)
    be = Backend(0.8, False, **kw)
    stems = [b"crowded_stem_%04d_%s" % (j, b"x" * (j % 50)) for j in range(600)]
    T = W.NOW0
    dead, keep = stems[0::3], [s for j, s in enumerate(stems) if j % 3]

    def batch(ss, unit, now, hits):
        n = len(ss)
        return arrays_from_lists(ss, [now] * n, list(range(n)), [unit] * n, [0] * n, [1000] * n, hits, [0] * n), n, n, 1

    # interleaved inserts: the dead keys (SECOND) lie between the kept ones (MINUTE) on the paths
    order = sorted(range(600), key=lambda j: (j * 7919) % 600)
    for lo in range(0, 600, 200):
        part = order[lo:lo + 200]
        d = [stems[j] for j in part if j % 3 == 0]
        k = [stems[j] for j in part if j % 3]
        be.do_limit_arrays(*batch(d, 1, T, [1] * len(d)), isolate=True)
        be.do_limit_arrays(*batch(k, 2, T + 5, [1 + stems.index(s) % 7 for s in k]), isolate=True)
    assert be.sweep(T + 10) == len(dead)
    return be, dead, keep, T + 10


def test_gpu_lookup_probes_past_tombstones_on_one_and_two_shards():
    be1, dead, keep, now = _crowd(1)
    be2 = _crowd(2)[0]
    try:
        assert be1.table_info()["tombstones"] == len(dead) == be2.table_info()["tombstones"]
        stems = keep + dead + [s + b"?" for s in keep[:100]]
        units = [2] * len(keep) + [1] * len(dead) + [2] * 100
        r1 = be1.lookup(stems, units, [now] * len(stems))
        r2 = be2.lookup(stems, units, [now] * len(stems))
        _all_ok(r1)
        nk = len(keep)
        assert r1["found"][:nk].all() and not r1["found"][nk:].any()
        all_stems = keep + dead
        want = [1 + (3 * (j // 2) + 1 + j % 2) % 7 for j in range(nk)]  # (keep[j] is stems[3 * (j // 2) + 1 + j % 2])
        assert list(r1["count"][:nk]) == want and (r1["expire"][:nk] == now - 5 + 60).all()
        assert len(set(all_stems)) == 600
        for k in abi.KEY_STATE_DTYPES:
            assert np.array_equal(r1[k], r2[k]), k  # key for key, whichever shard answered
    finally:
        be1.close()
        be2.close()


# --------------------------------------------------------------------------- 7. edges and validation
SENT8, SENT32 = 0xA5, 0xA5A5A5A5


def _raw(be, stems=None, units=None, nows=None, n=None, off=None, null=None, blob=None):
    """rl_lookup as a C caller makes it, the outputs pre-filled with a sentinel:
    -> (rc, outputs)."""
    stems = stems or []
    m = len(stems) if n is None else n
    if off is None:
        off = np.r_[0, np.cumsum([len(s) for s in stems])].astype(np.uint32)
    if blob is None:
        blob = np.frombuffer(b"".join(stems) or b"\0", np.uint8).copy()
    unit = np.ascontiguousarray(units if units is not None else [1] * m, np.uint8)
    now = np.ascontiguousarray(nows if nows is not None else [W.NOW0] * m, np.int64)
    out = {k: np.full(max(m, 1) + 4, SENT8 if dt == np.uint8 else SENT32, dt) for k, dt in abi.KEY_STATE_DTYPES.items()}
    k = abi.RlKeys()
    k.n = m
    k.stem_bytes, k.stem_off, k.unit, k.now = abi.ptr(blob), abi.ptr(off), abi.ptr(unit), abi.ptr(now)
    s = abi.RlKeyState()
    for f, v in out.items():
        setattr(s, f, None if f == null else abi.ptr(v))
    if null in ("stem_bytes", "stem_off", "unit", "now"):
        setattr(k, null, None)
    rc = be.L.rl_lookup(be.ctx, C.byref(k), C.byref(s))
    return rc, out


def _untouched(out, start=0):
    return all((v[start:] == (SENT8 if v.dtype == np.uint8 else SENT32)).all() for v in out.values())


def test_gpu_lookup_edges_and_validation():
    MB = 512
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=MB, max_rules=8, max_stem_bytes=1 << 17)
    try:
        stems = [b"edge_stem_%04d_" % j for j in range(MB + 1)]
        n_in = 300
        a = arrays_from_lists(stems[:n_in], [W.NOW0] * n_in, list(range(n_in)), [2] * n_in, [0] * n_in, [50] * n_in,
                              [1 + j % 3 for j in range(n_in)], [0] * n_in)
        be.do_limit_arrays(a, n_in, n_in, 1)
        for n in (0, 1, 256, 257, MB):
            rc, out = _raw(be, stems[:n], [2] * n)
            assert rc == abi.RL_OK, n
            assert _untouched(out, n), "wrote past n = %d" % n
            m = min(n, n_in)
            assert (out["status"][:n] == 0).all()
            assert out["found"][:m].all() and list(out["count"][:m]) == [1 + j % 3 for j in range(m)]
            assert not out["found"][m:n].any() and not out["count"][m:n].any()
        assert be.lookup([], [], [])["status"].size == 0
        # whole-call failures write nothing
        rc, out = _raw(be, stems[:MB + 1])
        assert rc == abi.RL_E_CAPACITY and _untouched(out)
        rc, out = _raw(be, [b"x" * 50_000] * 3)
        assert rc == abi.RL_E_CAPACITY and _untouched(out)
        for off in ([1, 4, 8], [0, 8, 4], [0, 4, 2]):
            rc, out = _raw(be, n=2, off=np.array(off, np.uint32), blob=np.zeros(16, np.uint8))
            assert rc == abi.RL_E_INVALID and _untouched(out), off
        for null in ("status", "found", "count", "expire", "lc", "stem_bytes", "stem_off", "unit", "now"):
            rc, out = _raw(be, stems[:3], null=null)
            assert rc == abi.RL_E_INVALID and _untouched(out), null
        assert be.L.rl_lookup(be.ctx, None, None) == abi.RL_E_INVALID
        with pytest.raises(RedisError, match="RL_E_INVALID"):
            be._check(_raw(be, stems[:3], null="lc")[0])
        # a key's own errors: its status only, the others answered
        mixed = [stems[0], stems[1], b"", stems[2], b"y" * 65536, stems[3], stems[4]]
        rc, out = _raw(be, mixed, [2, 0, 2, 5, 2, 2, 2])
        assert rc == abi.RL_OK
        assert list(out["status"][:7]) == [0, abi.RL_E_INVALID, abi.RL_E_INVALID, abi.RL_E_INVALID, abi.RL_E_INVALID, 0, 0]
        assert list(out["found"][:7]) == [1, 0, 0, 0, 0, 1, 1] and list(out["count"][:7]) == [1, 0, 0, 0, 0, 1, 2]
        assert not out["expire"][1:5].any() and not out["lc"][1:5].any() and _untouched(out, 7)
        rc, out = _raw(be, [b"z" * 65535], [2])  # the longest stem is a key like any other
        assert rc == abi.RL_OK and list(out["status"][:1]) == [0] and not out["found"][0]
    finally:
        be.close()


def test_gpu_lookup_refuses_a_communicator_ctx():
    from ratelimit_amd.sharded import loopback_id
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=64, max_rules=8)
    try:
        uid = loopback_id()
        be._check(be.L.rl_comm_init(be.ctx, 1, 0, abi.ptr(uid)))
        rc, out = _raw(be, [b"some_stem_"])
        assert rc == abi.RL_E_INVALID and _untouched(out)
    finally:
        be.close()


# --------------------------------------------------------------------------- peek
def test_gpu_peek_reads_what_do_limit_counted():
    lim = O.new_rate_limit(3, O.MINUTE, "peek_rule")
    req = O.RateLimitRequest("peek", [O.Descriptor([("user", "u1")]), O.Descriptor([("nil", "x")])], 2)
    now = M0 + 7
    cache = GpuRateLimitCache(FixedTimeSource(now), 0.8, True, cache_key_prefix="p:", table_slots=1 << 10,
                              max_batch=64, max_rules=8)
    try:
        assert cache.peek(req, [lim, None]) == [KeyState(0, None, False), None]
        cache.do_limit(None, req, [lim, None])
        assert cache.peek(req, [lim, None]) == [KeyState(2, 60, False), None]
        assert cache.peek(req, [lim, None]) == [KeyState(2, 60, False), None]  # (a peek counts nothing)
        cache.do_limit(None, req, [lim, None])  # 4 > 3: over, the local cache takes the key
        assert cache.peek(req, [lim, None], now=now + 1) == [KeyState(4, 59, True), None]
        assert cache.peek(req, [lim, None], now=M0 + 60) == [KeyState(0, None, False), None]  # the next minute's key
        with pytest.raises(RedisError, match="RL_E_TIME"):
            cache.peek(req, [lim, None], now=-5)
    finally:
        cache.close()
