"""rl_hot_keys: the k busiest and the currently blocked keys, selected on the GPU.

The call is defined against the export, so the oracle is a Python filter and
sort of Backend.export_records() on the same ctx: a key's record is the one
rl_export_range emits last for it (its newest window); it matches at `now`
when its unit is selected, ws == now - now % div, now <= expire, count >=
min_count and (blocked) now < lc. The answer holds every matching record above
its threshold, tied ones for the rest, count descending, then stem, then unit.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle
from oracle import oracle as O
from ratelimit_amd import abi, workloads as W
from ratelimit_amd.limiter import Backend, FixedTimeSource, GpuRateLimitCache, PinnedArena, RedisError
from ratelimit_amd.packing import PackedBatch, arrays_from_lists
from test_gpu_history import _stream
from test_gpu_migrate import _record_list
from test_gpu_observability import stream as obs_stream

pytestmark = pytest.mark.gpu

DIV = {1: 1, 2: 60, 3: 3600, 4: 86400}
NOW_MAX = 2 ** 32 - 172801


def _shards(n):
    return dict(n_shards=n, shard_devices=[0] * n) if n > 1 else {}


def _newest(be):
    """-> ([(stem, unit, ws, count, expire, lc)] one per key: the record the export
    emits last for it, slots summed over the shards)."""
    last, slots = {}, {}
    for part in be.export_records(1 << 12):
        slots[part["shard"]] = part["info"]["shard_slots"]
        for stem, unit, flags, ws, count, expire, lc in _record_list(part):
            last[(stem, unit)] = (stem, unit, ws, count, expire, lc)  # (a key's records: contiguous, oldest first)
    return list(last.values()), sum(slots.values())


def _order(r):
    return (-r[3], r[0], r[1])


def _matching(newest, now, units=None, min_count=0, blocked=False):
    """The oracle: the matching records, in the answer's order."""
    m = [r for r in newest if (not units or r[1] in units) and r[2] == now - now % DIV[r[1]] and now <= r[4]
         and r[3] >= min_count and (not blocked or now < r[5])]
    return sorted(m, key=_order)


def _answer(rec):
    assert not rec["flags"].any()
    return [(s, u, ws, c, e, lc) for s, u, f, ws, c, e, lc in _record_list(rec)]


def _check(be, newest, slots, now, k, units=None, min_count=0, blocked=False, m=None, mset=None):
    m = _matching(newest, now, units, min_count, blocked) if m is None else m
    mset = set(m) if mset is None else mset
    rec, info = be.hot_keys(now, k, min_count, units, blocked)
    got = _answer(rec)
    what = (now, k, units, min_count, blocked)
    n = min(k, len(m))
    assert len(got) == n, what
    assert [r[3] for r in got] == [r[3] for r in m[:n]], what  # the counts are the oracle's top k
    assert len(set(got)) == n and set(got) <= mset, what  # each a record of the export, every field and stem byte
    thr = m[n - 1][3] if n else 0
    above = [r for r in m[:n] if r[3] > thr]
    assert set(above) <= set(got), what  # every record above the threshold is there
    assert got == sorted(got, key=_order), what
    assert info == {"slots": slots, "matched": len(m), "hits": sum(r[3] for r in m), "above": len(above),
                    "threshold": thr, "time_floor": info["time_floor"]}, what
    return got, info


# --------------------------------------------------------------------------- 1. parity with the filtered export
MASKS = (None, (1,), (2,), (3, 4))


def _hot_stream(be, seed, tenants, nq):
    batches = _stream(seed, tenants, nq, 8, 3, 7, multi=True, hot=200)
    for x, n, q, nr in batches:
        g = be.do_limit_arrays(x, n, q, nr, isolate=True)
        assert (g["status"] == 0).all()
    return W.NOW0 + 7 * 3  # the last batch's clock


@pytest.mark.parametrize("slots,range_knob,tenants,nq", [(1 << 14, 1 << 10, 2500, 3000), (1 << 10, None, 120, 300)])
def test_gpu_hot_keys_equal_the_filtered_export(monkeypatch, slots, range_knob, tenants, nq):
    """2^14 slots scanned in ranges of 2^10 (the pool and the threshold cross
    range boundaries), and 2^10 slots in one range."""
    if range_knob:
        monkeypatch.setenv("RL_HOT_RANGE", str(range_knob))
    be = Backend(0.8, True, table_slots=slots, max_batch=1 << 13, max_rules=8, hash_seed=5, history_entries=1 << 16)
    try:
        T = _hot_stream(be, 31, tenants, nq)
        newest, n_slots = _newest(be)
        assert n_slots == slots and len(newest) > tenants
        some = 0
        for now in (T, T - 1, T + 86400):
            for units in MASKS:
                base = _matching(newest, now, units)
                top = base[0][3] if base else 1
                for min_count in (0, 2, top, top + 1):
                    m = [r for r in base if r[3] >= min_count]
                    mset = set(m)
                    for k in (0, 1, 63, 64, 65, 256, 257, 1025, len(m), len(m) + 1):
                        _check(be, newest, n_slots, now, k, units, min_count, m=m, mset=mset)
                    some += len(m) > 1025
        # (what keeps this test honest: answers cut from thousands of matching records on the larger table)
        assert some >= 2 if slots > 1 << 10 else len(_matching(newest, T)) > 64
        assert len(_matching(newest, T, (1,))) > 0 and len(_matching(newest, T, (2,))) > 64
    finally:
        be.close()


# --------------------------------------------------------------------------- 2. mass ties
def _one_each(stems, unit, now, hits, limit=1 << 30):
    n = len(stems)
    return arrays_from_lists(stems, [now] * n, list(range(n)), [unit] * n, [0] * n, [limit] * n, hits, [0] * n), n, n, 1


@pytest.mark.parametrize("range_knob", [None, 512])
def test_gpu_hot_keys_mass_ties(monkeypatch, range_knob):
    if range_knob:
        monkeypatch.setenv("RL_HOT_RANGE", str(range_knob))
    be = Backend(0.8, False, table_slots=1 << 13, max_batch=1 << 12, max_rules=8)
    try:
        T = W.NOW0 + 5
        ones = [b"tied_stem_%05d_" % j for j in range(3000)]
        five = [b"busier_stem_%d_" % j for j in range(5)]
        be.do_limit_arrays(*_one_each(ones + five, 2, T, [1] * 3000 + [2, 3, 4, 5, 6]))
        newest, slots = _newest(be)
        got, info = _check(be, newest, slots, T, 10)
        assert [r[3] for r in got] == [6, 5, 4, 3, 2, 1, 1, 1, 1, 1] and [r[0] for r in got[:5]] == five[::-1]
        assert info["threshold"] == 1 and info["above"] == 5 and info["matched"] == 3005 and info["hits"] == 3020
        got, info = _check(be, newest, slots, T, 3005)
        assert {r[0] for r in got} == set(ones + five) and info["above"] == 5
        for k in (5, 6, 2999, 3004):
            _check(be, newest, slots, T, k)
    finally:
        be.close()


# --------------------------------------------------------------------------- 3. radix digit boundaries
EDGES = [255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]


@pytest.mark.parametrize("range_knob", [None, 64])
def test_gpu_hot_keys_radix_digit_boundaries(monkeypatch, range_knob):
    if range_knob:
        monkeypatch.setenv("RL_HOT_RANGE", str(range_knob))
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=1 << 10, max_rules=8)
    try:
        T = W.NOW0 + 5
        stems = [b"edge_count_stem_%d_" % j for j in range(8)]
        be.restore(stems, [2] * 8, [T] * 8, EDGES)
        newest, slots = _newest(be)
        assert sorted(r[3] for r in newest) == EDGES
        for k in range(1, 9):
            got, info = _check(be, newest, slots, T, k)
            assert [r[3] for r in got] == EDGES[::-1][:k] and [r[0] for r in got] == stems[::-1][:k]
            assert info["threshold"] == EDGES[8 - k] and info["above"] == k - 1 and info["hits"] == sum(EDGES)
        for j, c in enumerate(EDGES):  # min_count on each boundary
            got, info = _check(be, newest, slots, T, 8, min_count=c)
            assert len(got) == 8 - j
    finally:
        be.close()


# --------------------------------------------------------------------------- 4. stems of every length
STEM_LENS = (1, 35, 36, 37, 52, 4096, 65535)


def test_gpu_hot_keys_stems_of_every_length():
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=64, max_rules=8, max_stem_bytes=1 << 18,
                 arena_bytes=1 << 19)
    try:
        T = W.NOW0 + 5
        stems = [bytes((7 * L + 13 * i) % 251 + 1 for i in range(L)) for L in STEM_LENS]
        stems += [s[:-1] + b"\xff" for s in stems[1:]]  # same head, another last byte (beyond a slot's 32 bytes)
        hits = [1 + j for j in range(len(stems))]
        be.do_limit_arrays(*_one_each(stems, 3, T, hits))
        assert be.table_info()["arena_bytes_used"] > 2 * 65535 - 64
        newest, slots = _newest(be)
        got, info = _check(be, newest, slots, T, 64)  # (140 KB of stems: hot_keys' retry with larger buffers)
        assert [r[0] for r in got] == stems[::-1] and [r[3] for r in got] == hits[::-1]
        got, _ = _check(be, newest, slots, T, 3)
        assert [r[0] for r in got] == stems[::-1][:3]
    finally:
        be.close()


# --------------------------------------------------------------------------- 5. the blocked list
def test_gpu_hot_keys_blocked_list_is_the_oracles_local_cache():
    """Single-unit stems: a freecache key is one window record. The keys
    (stem ‖ ws) answered with blocked=True at the last clock T are the Python
    oracle's local-cache keys live at T in T's own windows (an entry set in
    the minute before T outlives that window by its TTL, but no request at T
    reads it: ws != T - T % div, and rl_hot_keys reports windows at `now`)."""
    calls = obs_stream(7)
    oc = O.OracleFixedRateLimitCache(0.8, True)
    for r, l, now in calls:
        oc.do_limit(r, l, now)
    T = calls[-1][2]
    live_lc = {k for k, e in oc.client.data.items() if e[1] >= T and oc.local_cache.data.get(k, 0) > T}
    want = {k for k in live_lc if int(k[-10:]) in (T, T - T % 60)}  # (the stream's units: SECOND, MINUTE)
    assert len(live_lc) >= 10 and len(want) >= 10  # (what keeps this test honest)
    cache = GpuRateLimitCache(FixedTimeSource(T), 0.8, True, table_slots=1 << 12, max_batch=1 << 12, max_rules=1 << 10)
    try:
        for i in range(0, len(calls), 500):
            cache.do_limit_batch(calls[i:i + 500])
        got = cache.hot_keys(1000, blocked=True)
        keys = [h.stem.decode() + str(h.ws) for h in got]
        assert len(set(keys)) == len(keys) and set(keys) == want
        assert set(keys) <= live_lc and all(h.lc == oc.local_cache.data[k] for h, k in zip(got, keys))
        assert [h.count for h in got] == sorted((h.count for h in got), reverse=True)
        newest, slots = _newest(cache.backend)
        _check(cache.backend, newest, slots, T, 1000, blocked=True)
        _check(cache.backend, newest, slots, T, 7, blocked=True, min_count=2, units=(2,))
        every = cache.hot_keys(1000, now=T)
        assert set(keys) < {h.stem.decode() + str(h.ws) for h in every}
    finally:
        cache.close()
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=64, max_rules=8)
    try:
        with pytest.raises(RedisError, match="RL_E_INVALID"):
            be.hot_keys(T, 5, blocked=True)
        assert be.hot_keys(T, 5)[1]["matched"] == 0
    finally:
        be.close()


# --------------------------------------------------------------------------- 6. window semantics
def test_gpu_hot_keys_window_semantics_and_clock_errors():
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=64, max_rules=8)
    try:
        T = W.NOW0 // 60 * 60 + 60 + 30  # half way into a minute
        be.do_limit_arrays(*_one_each([b"hit_in_the_previous_window_"], 2, T - 31, [9]))
        be.do_limit_arrays(*_one_each([b"hit_in_a_later_window_"], 2, T + 60, [9]))
        be.do_limit_arrays(*_one_each([b"hit_now_"], 2, T - 1, [3]))
        # ws is T's window, but its EXPIRE has passed (a raw SET: rl_import keeps expire verbatim)
        stem = b"expired_in_its_window_"
        be.import_records({"stem_bytes": np.frombuffer(stem, np.uint8), "stem_off": np.array([0, len(stem)], np.uint32),
                           "unit": [2], "flags": [0], "ws": [T - 30], "count": [9], "expire": [T - 1], "lc": [0]})
        newest, slots = _newest(be)
        assert len(newest) == 4 and sorted(r[2] for r in newest) == [T - 90, T - 30, T - 30, T + 30]
        got, info = _check(be, newest, slots, T, 10)
        assert [r[0] for r in got] == [b"hit_now_"] and info["matched"] == 1 and info["hits"] == 3
        got, _ = _check(be, newest, slots, T - 1, 10)  # one second earlier the expired key was live
        assert [r[0] for r in got] == [stem, b"hit_now_"]
        got, _ = _check(be, newest, slots, T - 31, 10)
        assert [r[0] for r in got] == [b"hit_in_the_previous_window_"]
        got, _ = _check(be, newest, slots, T + 60, 10)
        assert [r[0] for r in got] == [b"hit_in_a_later_window_"]
        # the clock's range and the sweep floor
        assert be.hot_keys(NOW_MAX, 10)[1]["matched"] == 0 and be.hot_keys(0, 10)[1]["matched"] == 0
        for now in (NOW_MAX + 1, 2 ** 32, -1):
            with pytest.raises(RedisError, match="RL_E_TIME"):
                be.hot_keys(now, 10)
        be.sweep(T + 10)
        with pytest.raises(RedisError, match="RL_E_TIME"):
            be.hot_keys(T + 9, 10)
        rec, info = be.hot_keys(T + 10, 10)
        assert info["time_floor"] == T + 10 and info["matched"] == 1
    finally:
        be.close()


# --------------------------------------------------------------------------- 7. shards
def test_gpu_hot_keys_on_two_and_three_shards():
    """Every shard answers its own top k, the host merges them: the same records
    and info as one shard. Forty keys with distinct counts above everything else
    lead, so that ties cannot differ where records are compared."""
    res = {}
    for n in (1, 2, 3):
        be = Backend(0.8, True, table_slots=1 << 14, max_batch=1 << 13, max_rules=8, hash_seed=5,
                     history_entries=1 << 16, **_shards(n))
        try:
            T = _hot_stream(be, 31, 2500, 3000)
            lead = [b"leading_stem_%02d_" % j for j in range(40)]
            be.do_limit_arrays(*_one_each(lead, 2, T, [5000 + 7 * j for j in range(40)]))
            newest, slots = _newest(be)
            n_match = len(_matching(newest, T))
            out = {}
            for k in (1, 10, 40, 300, n_match, n_match + 1):
                got, info = _check(be, newest, slots, T, k)
                info.pop("slots")
                out[k] = (got if k <= 40 or k >= n_match else sorted(r[3] for r in got), info)
            out["blocked"] = _check(be, newest, slots, T, n_match, blocked=True)[0]
            out["minute"] = _check(be, newest, slots, T, 40, units=(2,), min_count=5000)[0]
            res[n] = out
        finally:
            be.close()
    assert [r[0] for r in res[1][40][0]] == [b"leading_stem_%02d_" % j for j in range(39, -1, -1)]
    assert len(res[1]["blocked"]) > 0 and len(res[1]["minute"]) == 40
    assert res[2] == res[1] and res[3] == res[1]


# --------------------------------------------------------------------------- 8. read-only and ordered
def test_gpu_hot_keys_change_nothing_and_order_after_batches():
    batches = _stream(33, 1500, 2000, 8, 3, 7, multi=True, hot=200)
    be = Backend(0.8, True, table_slots=1 << 14, max_batch=1 << 13, max_rules=8, history_entries=1 << 16)
    co = c_oracle.COracle(0.8, True)

    def play(part, base):
        for i, (x, n, nq, nr) in enumerate(part):
            g, o = be.do_limit_arrays(x, n, nq, nr, isolate=True), co.do_limit(x, n, nq, nr)
            assert (g["status"] == 0).all()
            for f in ("code", "limit_remaining", "reset_s", "stats"):
                assert np.array_equal(g[f], o[f]), (base + i, f)

    try:
        play(batches[:4], 0)
        T = W.NOW0 + 3 * 3

        def readings():
            return be.snapshot().tobytes(), be.table_info(), be.local_cache_info(T)

        before = readings()
        assert before[1]["history_slots"] > 0 and before[2]["entry_count"] > 0
        n_got = 0
        for k, kw in ((0, {}), (10, {}), (5000, {}), (100, dict(blocked=True)), (64, dict(units=(1,), min_count=2)),
                      (10, dict(now=T - 2)), (10, dict(now=T + 86400))):
            n_got += len(be.hot_keys(kw.pop("now", T), k, **kw)[0]["ws"])
        assert n_got > 1000
        after = readings()
        assert before[1] == after[1], "table_info changed"
        assert before[2] == after[2], "local-cache gauges changed"
        assert before[0] == after[0], "the snapshot changed"
        play(batches[4:6], 4)  # and the stream goes on bit-exactly
        # batches submitted and not yet synchronised are visible to the call
        arena = PinnedArena()
        keep = []
        for x, n, nq, nr in batches[6:]:
            pb = PackedBatch({f: arena.like(v) for f, v in x.items()}, n, nq, nr)
            out = {f: arena.like(v) for f, v in pb.alloc_result(True).items()}
            keep.append((pb, out, be.do_limit_host_async(pb, out)))
        T = W.NOW0 + 7 * 3
        rec, info = be.hot_keys(T, 1 << 13)  # (no synchronize in between)
        be.synchronize()
        for (pb, out, _), (x, n, nq, nr) in zip(keep, batches[6:]):
            o = co.do_limit(x, n, nq, nr)
            assert not out["status"][:n].any() and np.array_equal(out["code"][:n], o["code"])
        newest, slots = _newest(be)
        m = _matching(newest, T)
        assert sorted(_answer(rec), key=_order) == m and info["matched"] == len(m) > 100
        arena.close()
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 9. errors write nothing
SENT8, SENT32 = 0xA5, 0xA5A5A5A5


def _raw(be, now, k, n_cap, stem_cap, mask=0, flags=0, min_count=0, null=None, no_q=False, no_info=False):
    """rl_hot_keys as a C caller makes it, `out` pre-filled with a sentinel -> (rc, out arrays, rl_records, info)."""
    bufs = {"stem_bytes": np.full(max(stem_cap, 1) + 8, SENT8, np.uint8), "stem_off": np.full(n_cap + 5, SENT32, np.uint32)}
    for f, dt in abi.RECORD_DTYPES.items():
        bufs[f] = np.full(n_cap + 4, SENT8 if dt == np.uint8 else SENT32, dt)
    q = abi.RlHotQuery()
    q.now, q.k, q.min_count, q.unit_mask, q.flags = now, k, min_count, mask, flags
    r = abi.RlRecords()
    r.n, r.stem_cap = n_cap, stem_cap
    for f, v in bufs.items():
        setattr(r, f, None if f == null else abi.ptr(v))
    info = abi.RlHotInfo()
    rc = be.L.rl_hot_keys(be.ctx, None if no_q else C.byref(q), None if null == "out" else C.byref(r),
                          None if no_info else C.byref(info))
    return rc, bufs, r, info


def _untouched(bufs, r, n_cap, stem_cap):
    return all((v == (SENT8 if v.dtype == np.uint8 else SENT32)).all() for v in bufs.values()) and \
        (r.n, r.stem_cap) == (n_cap, stem_cap)


def test_gpu_hot_keys_errors_write_nothing():
    MB = 256
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=MB, max_rules=8)
    try:
        T = W.NOW0 + 5
        stems = [b"error_case_stem_%03d_" % j for j in range(100)]
        nb = sum(len(s) for s in stems)
        be.do_limit_arrays(*_one_each(stems, 2, T, [1 + j for j in range(100)]))
        rc, bufs, r, info = _raw(be, T, 100, 100, nb)  # exactly what the answer needs
        assert rc == abi.RL_OK and r.n == 100 and bufs["stem_off"][100] == nb and list(bufs["count"][:3]) == [100, 99, 98]
        assert (bufs["stem_off"][101:] == SENT32).all() and (bufs["count"][100:] == SENT32).all()
        assert (bufs["stem_bytes"][nb:] == SENT8).all() and not bufs["flags"][:100].any()
        bad = dict(
            unknown_flags=dict(flags=2), flags_and_blocked=dict(flags=3), mask_bit_0=dict(mask=1), mask_bit_5=dict(mask=1 << 5),
            mask_high=dict(mask=1 << 31), blocked_without_local_cache=dict(flags=abi.RL_HOT_BLOCKED),
            null_out=dict(null="out"), null_count=dict(null="count"), null_stem_off=dict(null="stem_off"),
            null_stem_bytes=dict(null="stem_bytes"), null_q=dict(no_q=True), null_info=dict(no_info=True))
        for name, kw in bad.items():
            rc, bufs, r, info = _raw(be, T, 10, 100, nb, **kw)
            assert rc == abi.RL_E_INVALID and _untouched(bufs, r, 100, nb), name
        rc, bufs, r, info = _raw(be, T, MB + 1, MB + 1, 1 << 16)
        assert rc == abi.RL_E_CAPACITY and _untouched(bufs, r, MB + 1, 1 << 16) and info.matched == 0
        assert _raw(be, T, MB, MB, 1 << 16)[0] == abi.RL_OK
        # capacity short by one record, by one stem byte: nothing written, info says what is needed
        for n_cap, stem_cap in ((99, nb), (100, nb - 1), (0, 0)):
            rc, bufs, r, info = _raw(be, T, 100, n_cap, stem_cap)
            assert rc == abi.RL_E_CAPACITY and _untouched(bufs, r, n_cap, stem_cap), (n_cap, stem_cap)
            assert (info.matched, info.hits, info.threshold, info.above, info.slots) == (100, 5050, 1, 99, 1 << 10)
        rc, bufs, r, info = _raw(be, T, 30, 30, nb, min_count=51)  # fewer match than k: min(k, matched) records
        assert rc == abi.RL_OK and r.n == 30 and info.matched == 50
        rc, bufs, r, info = _raw(be, T, 0, 0, 0, null="out")  # k = 0: only info, out may be null
        assert rc == abi.RL_OK and info.matched == 100 and info.threshold == 0 and info.above == 0
        for now in (-1, NOW_MAX + 1):
            rc, bufs, r, info = _raw(be, now, 10, 100, nb)
            assert rc == abi.RL_E_TIME and _untouched(bufs, r, 100, nb)
        with pytest.raises(RedisError, match="unit_mask.*RL_E_INVALID"):
            be._check(_raw(be, T, 10, 100, nb, mask=1)[0])
    finally:
        be.close()


def test_gpu_hot_keys_refuse_a_communicator_ctx():
    from ratelimit_amd.sharded import loopback_id
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=64, max_rules=8)
    try:
        uid = loopback_id()
        be._check(be.L.rl_comm_init(be.ctx, 1, 0, abi.ptr(uid)))
        rc, bufs, r, info = _raw(be, W.NOW0, 10, 16, 1 << 10)
        assert rc == abi.RL_E_INVALID and _untouched(bufs, r, 16, 1 << 10)
    finally:
        be.close()
