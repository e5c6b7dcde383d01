"""rl_scan on the GPU: keys listed by stem prefix, page by page (Backend.scan,
Backend.count_keys, GpuRateLimitCache.list_keys).

The scan is defined against the export, so the expected answer is a filter of
Backend.export_records() written out in Python (scan_cases.expected: group by
(stem, unit), the prefix / unit / NEWEST / LIVE rules and the flag rule of
include/ratelimit_hip.h). The table holds the first half of test_gpu_forget's
stream, which has stems under two units, long stems, history chains, expired
and live records and two domains of which one's name begins the other's
(tests/test_scan_cpu.py shows that with the oracle alone), plus the stems cut at
the slot layout's edges.
"""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O
from ratelimit_amd import abi, workloads as W
from ratelimit_amd.limiter import Backend, FixedTimeSource, GpuRateLimitCache, PinnedArena
from ratelimit_amd.packing import PackedBatch, arrays_from_lists
import scan_cases as SC
from test_gpu_forget import SMALL, fg_stream, insert, run_gpu

pytestmark = pytest.mark.gpu

TILE = abi.RL_SCAN_TILE
NEWEST, LIVE = abi.RL_SCAN_NEWEST, abi.RL_SCAN_LIVE
CONFIGS = [(False, False), (True, False), (False, True), (True, True)]  # (local cache, per_second)
SENT = 0xA5


def key_counts(recs):
    """The multiset of records."""
    out = {}
    for r in recs:
        out[r] = out.get(r, 0) + 1
    return out


# --------------------------------------------------------------------------- the tables, built once
_CALLS = fg_stream(5)
_HALF = len(_CALLS) // 2
T = _CALLS[_HALF][2]
_tables = {}


def stream_table(local_cache, per_second, n_shards=1):
    """A cache after the stream's first half and the edge stems (MINUTE, at T),
    its export in the export's order, and the oracle after the same calls.
    Shared by the tests that only read."""
    key = (local_cache, per_second, n_shards)
    if key not in _tables:
        kw = dict(n_shards=n_shards, shard_devices=[0] * n_shards) if n_shards > 1 else {}
        cache = GpuRateLimitCache(FixedTimeSource(T), 0.8, local_cache, per_second=per_second, **SMALL, **kw)
        run_gpu(cache, _CALLS[:_HALF])
        insert(cache.backend, SC.edge_stems(), unit=2, now=T, hits=3)
        oc = O.OracleFixedRateLimitCache(0.8, local_cache, per_second=per_second)
        for r, l, now in _CALLS[:_HALF]:
            oc.do_limit(r, l, now)
        _tables[key] = (cache, SC.export_list(cache.backend), oc)
    return _tables[key]


@pytest.fixture(scope="module", autouse=True)
def _close_tables():
    yield
    for cache, _, _ in _tables.values():
        cache.close()
    _tables.clear()


def check_query(be, export, **kw):
    """One query over all pages against the filter of the export."""
    want, winfo, wbyp = SC.expected(export, **kw)
    got, ginfo, gbyp, pages = SC.scan_all(be, **kw)
    SC.groups_of(got)  # every key's records contiguous and oldest first, no key twice
    assert key_counts(got) == key_counts(want), (kw, len(got), len(want))
    for f, v in winfo.items():
        assert ginfo[f] == v, (f, kw)
    assert gbyp == wbyp, kw
    return want, winfo, wbyp


# --------------------------------------------------------------------------- 1. content against the export
@pytest.mark.parametrize("local_cache,per_second", CONFIGS)
def test_gpu_scan_equals_the_filtered_export(local_cache, per_second):
    cache, export, _ = stream_table(local_cache, per_second)
    be = cache.backend
    assert len(export) > 300 and any(len(g) > 1 for g in SC.groups_of(export))
    assert any(r[5] < T for r in export) and any(r[5] >= T for r in export)  # expired and live at T
    p64 = SC.p64()
    # no prefix: the whole export, record for record
    want, info, _ = check_query(be, export)
    assert key_counts(want) == key_counts(export) and info["keys"] == be.table_info()["live_slots"]
    # one domain; both ("fg_" begins "fg_b_" too)
    w_fg, i_fg, _ = check_query(be, export, prefixes=SC.DOMAIN)
    w_both, i_both, _ = check_query(be, export, prefixes=SC.BOTH)
    assert 0 < i_fg["keys"] < i_both["keys"] < info["keys"]
    # 64 prefixes: overlapping, 1 / 3 / 4 / 5 bytes, 32 / 33 / 36 / 37, a whole stem, one byte more, never seen
    w64, i64, b64 = check_query(be, export, prefixes=p64)
    keys64 = [b[0] for b in b64]
    assert keys64[0] == 1 and keys64[1] == 0 and keys64[2] > 0 and keys64[3] == 0 and keys64[8] == 0
    assert keys64[7] == 1 and keys64[9] == 2 and all(k > 0 for k in keys64[10:19]) and not any(keys64[19:])
    assert 0 < i64["keys"] < info["keys"]
    # each unit-mask bit, alone and under the prefixes
    per_unit = 0
    for u in (1, 2, 3, 4):
        _, iu, _ = check_query(be, export, units=[u])
        assert iu["keys"] > 0, u
        per_unit += iu["keys"]
        check_query(be, export, prefixes=p64, units=[u])
    assert per_unit == info["keys"]
    _, i24, _ = check_query(be, export, prefixes=SC.BOTH, units=[2, 4])
    assert 0 < i24["keys"] < i_both["keys"]
    # NEWEST, LIVE at T, both
    for prefixes in ((), SC.DOMAIN, p64):
        _, i_new, _ = check_query(be, export, prefixes=prefixes, newest=True)
        _, i_live, _ = check_query(be, export, prefixes=prefixes, now=T)
        _, i_nl, _ = check_query(be, export, prefixes=prefixes, newest=True, now=T)
        _, i_all, _ = check_query(be, export, prefixes=prefixes)
        assert i_new["keys"] == i_all["keys"] == i_new["records"] < i_all["records"]  # one record per key
        assert 0 < i_nl["records"] <= i_live["records"] < i_all["records"]
        # keys left without a record are no keys of the answer: 90 s on, no SECOND or MINUTE record is live
        _, i_late, _ = check_query(be, export, prefixes=prefixes, now=T + 90)
        assert 0 < i_late["keys"] < i_all["keys"] and i_late["keys"] <= i_live["keys"] <= i_all["keys"]
        assert i_new["chains_lost"] == 0
    # a clock past every expiry: the empty answer
    far = max(r[5] for r in export) + 1
    got, ginfo, gbyp, _ = SC.scan_all(be, prefixes=SC.BOTH, now=far)
    assert got == [] and not any(ginfo[f] for f in ("keys", "records", "stem_bytes")) and gbyp == [[0, 0, 0]]


def test_gpu_scan_flags_lost_chains_as_the_export_does():
    """The smallest history log under a 600 s horizon, 1000 SECOND keys rolled
    through 120 windows (test_gpu_migrate's recipe): every partition wraps, so
    many chain walks break. The scan marks exactly the keys the export marks, on
    the first record it emits for them (after the LIVE filter too), never with
    NEWEST, and counts them in chains_lost."""
    be = Backend(0.8, True, history_entries=1, table_slots=1 << 14, max_batch=1 << 11, max_rules=8, jitter=600)
    try:
        for k in range(120):
            a, n, nq, nr = W.c1_batch(np.arange(500), W.NOW0 + k)
            a["unit"][:] = 1  # both stems of a tenant under SECOND: 1000 single-unit keys
            assert (be.do_limit_arrays(a, n, nq, nr, isolate=True)["status"] == 0).all()
        export = SC.export_list(be)
        lost = sum(1 for g in SC.groups_of(export) if g[0][2] & abi.RL_REC_CHAIN_LOST)
        assert 0 < lost and len(export) > 5000
        _, info, _ = check_query(be, export)
        assert info["chains_lost"] == lost
        some = [b"bench_tenant_t00000001", b"bench_tenant_t000000002"]
        _, i_some, _ = check_query(be, export, prefixes=some)
        assert 0 < i_some["keys"] < 1000
        exp = sorted(r[5] for r in export)
        assert exp[0] < exp[len(exp) // 3] < exp[-1]
        for now in (exp[len(exp) // 3], exp[2 * len(exp) // 3], exp[-1]):  # fewer and fewer records are live:
            # the flag moves to the first one left
            _, i_live, _ = check_query(be, export, now=now)
            check_query(be, export, prefixes=some, now=now)
            assert 0 < i_live["records"] < info["records"]
        assert i_live["chains_lost"] > 0
        _, i_new, _ = check_query(be, export, newest=True)
        assert i_new["chains_lost"] == 0 and i_new["records"] == 1000
        got, ginfo, _, pages = SC.scan_all(be, page_records=4096)  # (several pages of many-record keys)
        assert pages > 1 and key_counts(got) == key_counts(export) and ginfo["chains_lost"] == lost
    finally:
        be.close()


# --------------------------------------------------------------------------- 2. against the Python oracle
@pytest.mark.parametrize("local_cache,per_second", CONFIGS)
def test_gpu_scan_live_keys_are_the_oracles(local_cache, per_second):
    """The (stem ‖ decimal(ws), count) pairs under the prefix "fg_" and, alone,
    under the domain "fg": with LIVE they are exactly the keys that exist in
    the oracle's client / per_second_client stores at T; with NEWEST | LIVE
    exactly those among them that are their (stem, unit)'s newest window. (A
    key's older window may still be live at T beside its newest: MINUTE keys
    live 60 s past their last hit. NEWEST returns the last record only, so the
    bare NEWEST | LIVE answer is a subset of the store, the store's keys whose
    window is the newest; both directions are checked.) Where a stem's unit
    slots alias one Redis key (their windows coincide in one store), the first
    record in unit order stands for the key, rl_lookup's rule."""
    cache, export, oc = stream_table(local_cache, per_second)
    be = cache.backend

    def store_of(unit):
        return 1 if per_second and unit == 1 else 0

    def pairs(recs):
        out = {}
        for r in sorted(recs, key=lambda r: r[1]):  # unit order: the first record of a Redis key stands
            out.setdefault((store_of(r[1]), r[0].decode() + str(r[3])), r[4])
        return out

    stores = [oc.client.data, oc.per_second_client.data if per_second else {}]
    for prefixes in (SC.BOTH, SC.DOMAIN):
        p = prefixes[0].decode()
        want = {(i, k): e[0] for i, s in enumerate(stores) for k, e in s.items() if k.startswith(p) and T <= e[1]}
        assert len(want) > 10 and len(want) < sum(len(s) for s in stores)  # (most of the stores' keys have expired)
        got, _, _, _ = SC.scan_all(be, prefixes=prefixes, now=T)
        assert pairs(got) == want
        newest_ws = {}
        for g in SC.groups_of([r for r in export if r[0].startswith(prefixes[0])]):
            newest_ws[(store_of(g[0][1]), g[0][0].decode(), g[0][1])] = g[-1][3]
        got_nl, _, _, _ = SC.scan_all(be, prefixes=prefixes, now=T, newest=True)
        assert all(newest_ws[(store_of(r[1]), r[0].decode(), r[1])] == r[3] for r in got_nl)
        want_nl = {}
        for (st, stem, unit), ws in sorted(newest_ws.items(), key=lambda kv: kv[0][2]):
            if (st, stem + str(ws)) in want:
                want_nl.setdefault((st, stem + str(ws)), want[(st, stem + str(ws))])
        assert pairs(got_nl) == want_nl and 0 < len(want_nl) <= len(want)


# --------------------------------------------------------------------------- 3. against rl_forget's dry run
def test_gpu_scan_by_prefix_keys_equal_forgets_dry_run():
    cache, export, _ = stream_table(True, False)
    be = cache.backend
    p64 = SC.p64()
    dry = be.forget(p64, prefix=True, dry_run=True)
    _, info, byp, _ = SC.scan_all(be, prefixes=p64)
    assert [b[0] for b in byp] == dry["removed"].tolist() and info["keys"] == dry["keys"] > 0
    cnt = be.count_keys(p64)
    assert cnt["by_prefix"][:, 0].tolist() == dry["removed"].tolist() and cnt["by_prefix"].tolist() == byp
    assert cnt["slots_scanned"] == dry["slots_scanned"] == SMALL["table_slots"]


# --------------------------------------------------------------------------- raw calls
def raw_scan(be, prefixes=(), flags=0, now=0, unit_mask=0, cur=(0, 0), n_cap=1 << 12, stem_cap=1 << 18, out=True,
             info=True, byp=True, q_reserved=0, cur_reserved=0, off=None, null=None, n_prefixes=None):
    """rl_scan as a C caller makes it, every output pre-filled with a sentinel.
    -> dict(rc, cur, recs, info words, byp words, untouched: no output byte moved)."""
    prefixes = list(prefixes)
    n = len(prefixes) if n_prefixes is None else n_prefixes
    if off is None:
        off = np.r_[0, np.cumsum([len(p) for p in prefixes])].astype(np.uint32)
    blob = np.frombuffer(b"".join(prefixes) or b"\0", np.uint8).copy()
    q = abi.RlScanQuery()
    q.n_prefixes, q.flags, q.now, q.unit_mask, q.reserved = n, flags, now, unit_mask, q_reserved
    q.prefix_bytes = None if null == "prefix_bytes" else abi.ptr(blob)
    q.prefix_off = None if null == "prefix_off" else abi.ptr(off)
    c = abi.RlScanCursor()
    c.shard, c.slot, c.reserved = cur[0], cur[1], cur_reserved
    bufs = {"stem_bytes": np.full(max(stem_cap, 1) + 8, SENT, np.uint8),
            "stem_off": np.full(n_cap + 1 + 2, 0xA5A5A5A5, np.uint32)}
    for k, dt in abi.RECORD_DTYPES.items():
        bufs[k] = np.full(n_cap + 2, SENT if dt == np.uint8 else 0xA5A5A5A5, dt)
    r = abi.RlRecords()
    r.n, r.stem_cap = n_cap, stem_cap
    for k, v in bufs.items():
        setattr(r, k, None if null == k else abi.ptr(v))
    iw = np.full(8, 0xA5A5A5A5A5A5A5A5, np.uint64)
    bw = np.full((max(n, 1) + 1, 3), 0xA5A5A5A5A5A5A5A5, np.uint64)
    rc = be.L.rl_scan(be.ctx, None if null == "q" else C.byref(q), None if null == "cur" else C.byref(c),
                      C.byref(r) if out else None, abi.ptr(bw) if byp else None,
                      C.cast(abi.ptr(iw), C.POINTER(abi.RlScanInfo)) if info else None)
    sent = {k: v == (SENT if v.dtype == np.uint8 else 0xA5A5A5A5) for k, v in bufs.items()}  # still the sentinel
    res = dict(rc=rc, cur=(int(c.shard), int(c.slot)), info=iw, byp=bw, n=int(r.n), bufs=bufs, sent=sent)
    res["untouched"] = bool(all(s.all() for s in sent.values()) and (iw == 0xA5A5A5A5A5A5A5A5).all() and
                            (bw == 0xA5A5A5A5A5A5A5A5).all() and r.n == n_cap and res["cur"] == tuple(cur))
    if rc == abi.RL_OK and out:
        m = int(r.n)
        nb = int(bufs["stem_off"][m])
        rec = {k: bufs[k][:m] for k in abi.RECORD_DTYPES}
        rec["stem_off"], rec["stem_bytes"] = bufs["stem_off"][:m + 1], bufs["stem_bytes"][:nb]
        res["recs"] = SC.rec_list(rec)
        res["raw"] = b"".join(bufs[k][:m].tobytes() for k in abi.RECORD_DTYPES) + bufs["stem_off"][:m + 1].tobytes() + \
            bufs["stem_bytes"][:nb].tobytes()
        # nothing past what the call says it wrote
        assert all(sent[k][m:].all() for k in abi.RECORD_DTYPES) and sent["stem_off"][m + 1:].all()
        assert sent["stem_bytes"][nb:].all() and (bw[max(n, 1):] == 0xA5A5A5A5A5A5A5A5).all()
    return res


INFO_F = [f for f, _ in abi.RlScanInfo._fields_]


def info_of(res):
    d = dict(zip(INFO_F, (int(x) for x in res["info"])))
    return d


# --------------------------------------------------------------------------- 4. paging
def paging_stems(n):
    """n stems, one in 97 under "pg_03_", one in ten under "pg_5"; every seventh
    is longer than the slot's inline bytes."""
    return [b"pg_%02d_%05d_" % (j % 97, j) + (b"long_tail_" * 4 if j % 7 == 3 else b"") for j in range(n)]


@pytest.mark.parametrize("slots", [256, 1024, 2048, 1 << 14])
def test_gpu_scan_pages_concatenate_to_the_one_call_answer(slots):
    """Tables below one tile, of exactly one, of two and of many, filled to 0.6
    (every tile edge is populated); a tenth of the keys get a second window.
    Pages of 1, 7 and 64 records and of few stem bytes: the concatenation is
    byte for byte the one-call answer, cursors are tile multiples (or the
    shard's end) and rise, a first tile that does not fit is RL_E_CAPACITY with
    nothing written, and a retry with need_* succeeds. Every key appears
    exactly once."""
    be = Backend(0.8, False, table_slots=slots, max_batch=1 << 12, max_rules=8)
    try:
        stems = paging_stems(int(slots * 0.6))
        for lo in range(0, len(stems), 1 << 12):
            insert(be, stems[lo:lo + (1 << 12)], unit=2, now=T)
        again = stems[::10]
        for lo in range(0, len(again), 1 << 12):
            insert(be, again[lo:lo + (1 << 12)], unit=2, now=T + 60)
        export = SC.export_list(be)
        ntiles = (slots + TILE - 1) // TILE
        for prefixes in ([], [b"pg_03_", b"pg_5"]):
            want, winfo, wbyp = SC.expected(export, prefixes=prefixes)
            one = raw_scan(be, prefixes, n_cap=1 << 15, stem_cap=1 << 21)
            assert one["rc"] == abi.RL_OK and one["cur"] == (1, 0)
            assert key_counts(one["recs"]) == key_counts(want) and len(want) > 0
            assert len({r[:2] for r in want}) == winfo["keys"]
            assert info_of(one)["slots_scanned"] == slots and info_of(one)["records"] == len(want)
            for n_cap, stem_cap in ((1, 1 << 20), (7, 1 << 20), (64, 1 << 20), (1 << 15, 40), (1 << 15, 700),
                                    (64, 700)):
                cur, recs, raws, calls, refused = (0, 0), [], [], 0, 0
                sums = {f: 0 for f in ("slots_scanned", "keys", "records", "stem_bytes", "chains_lost")}
                byp = np.zeros((max(len(prefixes), 1), 3), np.int64)
                bound = {"rec": 0, "byte": 0}
                while cur[0] == 0:
                    res = raw_scan(be, prefixes, cur=cur, n_cap=n_cap, stem_cap=stem_cap)
                    calls += 1
                    assert calls <= 2 * ntiles + 2
                    if res["rc"] == abi.RL_E_CAPACITY:
                        i = info_of(res)
                        need = (i["need_records"], i["need_stem_bytes"])
                        assert need[0] > n_cap or need[1] > stem_cap
                        assert all(s.all() for s in res["sent"].values()) and res["cur"] == cur and res["n"] == n_cap
                        assert (res["byp"] == 0xA5A5A5A5A5A5A5A5).all()
                        bound["rec" if need[0] > n_cap else "byte"] += 1
                        refused += 1
                        res = raw_scan(be, prefixes, cur=cur, n_cap=max(n_cap, need[0]), stem_cap=max(stem_cap, need[1]))
                        i2 = info_of(res)
                        # the retry covers that tile (what it needs fits exactly) and whatever fits after it
                        assert res["rc"] == abi.RL_OK and i2["records"] >= need[0] and i2["stem_bytes"] >= need[1]
                    assert res["rc"] == abi.RL_OK
                    nxt = res["cur"]
                    assert nxt > cur and (nxt == (1, 0) or (nxt[0] == 0 and nxt[1] % TILE == 0 and nxt[1] < slots))
                    i = info_of(res)
                    end = slots if nxt[0] else nxt[1]
                    assert i["slots_scanned"] == end - cur[1] and i["records"] == len(res["recs"])
                    assert i["need_records"] == 0 == i["need_stem_bytes"]
                    recs += res["recs"]
                    raws.append(res)
                    for f in sums:
                        sums[f] += i[f]
                    byp += res["byp"][:len(byp)].astype(np.int64)
                    cur = nxt
                assert cur == (1, 0)
                # byte-identical: the same records in the same order, the stem offsets restarting per page
                assert recs == one["recs"], (n_cap, stem_cap)
                for f in abi.RECORD_DTYPES:
                    assert b"".join(r["bufs"][f][:len(r["recs"])].tobytes() for r in raws) == \
                        one["bufs"][f][:len(recs)].tobytes(), f
                nb = lambda r: int(r["bufs"]["stem_off"][len(r["recs"])])
                assert b"".join(r["bufs"]["stem_bytes"][:nb(r)].tobytes() for r in raws) == \
                    one["bufs"]["stem_bytes"][:nb(one)].tobytes()
                assert len({r[:2] for r in recs}) == winfo["keys"] == sums["keys"]  # every key, each once
                for f, v in winfo.items():
                    assert sums[f] == v, f
                assert byp.tolist() == wbyp
                if slots > TILE and prefixes and (n_cap, stem_cap) in ((7, 1 << 20), (64, 1 << 20), (1 << 15, 700)):
                    assert len(raws) > 1  # (more than one page)
                if (n_cap, stem_cap) == (1, 1 << 20):
                    assert bound["rec"] > 0 and bound["byte"] == 0
                if (n_cap, stem_cap) == (1 << 15, 40):
                    assert bound["byte"] > 0 and bound["rec"] == 0
    finally:
        be.close()


def test_gpu_scan_caps_bind_across_tiles():
    """Capacities between one tile's need and the whole answer: the record cap
    ends one page, the byte cap another, exactly in front of the first tile that
    does not fit (the planner's cut, on the device's tile sums)."""
    slots = 1 << 14
    be = Backend(0.8, False, table_slots=slots, max_batch=1 << 12, max_rules=8)
    try:
        stems = paging_stems(int(slots * 0.6))
        for lo in range(0, len(stems), 1 << 12):
            insert(be, stems[lo:lo + (1 << 12)], unit=2, now=T)
        prefixes = [b"pg_03_", b"pg_5"]
        tiles = []
        for t in range(slots // TILE):  # each tile's own sums: a count-only call covers the rest of the shard
            a = info_of(raw_scan(be, prefixes, cur=(0, t * TILE), out=False))
            b = info_of(raw_scan(be, prefixes, cur=(0, (t + 1) * TILE), out=False)) if t + 1 < slots // TILE else None
            tiles.append((a["records"] - (b["records"] if b else 0), a["stem_bytes"] - (b["stem_bytes"] if b else 0)))
        assert all(r > 0 for r, _ in tiles)
        r3, b3 = sum(r for r, _ in tiles[:3]), sum(b for _, b in tiles[:3])
        # records bind: three tiles fit exactly, one record less covers two
        for n_cap, stem_cap, covered in ((r3, 1 << 20, 3), (r3 - 1, 1 << 20, 2), (1 << 15, b3, 3), (1 << 15, b3 - 1, 2),
                                         (r3 + tiles[3][0] - 1, b3, 3), (r3, b3 + tiles[3][1] - 1, 3)):
            res = raw_scan(be, prefixes, n_cap=n_cap, stem_cap=stem_cap)
            assert res["rc"] == abi.RL_OK and res["cur"] == (0, covered * TILE), (n_cap, stem_cap)
            assert info_of(res)["records"] == sum(r for r, _ in tiles[:covered])
            assert info_of(res)["stem_bytes"] == sum(b for _, b in tiles[:covered])
    finally:
        be.close()


@pytest.mark.parametrize("span", [1, 3])
def test_gpu_scan_spans_join_seamlessly(span, monkeypatch):
    """A call counts its tiles in spans (RL_SCAN_SPAN caps them: here 1 and 3
    tiles, on a table of 16): the answer of a ctx with tiny spans is byte for
    byte that of a ctx with the default ones, for one call over everything and
    for pages that end inside a span and at its edge."""
    slots = 1 << 14
    stems = paging_stems(int(slots * 0.6))
    bes = []
    try:
        a = Backend(0.8, False, table_slots=slots, max_batch=1 << 12, max_rules=8, hash_seed=5)
        bes.append(a)
        for lo in range(0, len(stems), 1 << 12):
            insert(a, stems[lo:lo + (1 << 12)], unit=2, now=T)
        monkeypatch.setenv("RL_SCAN_SPAN", str(span))  # (read when a ctx is created)
        b = Backend(0.8, False, table_slots=slots, max_batch=1 << 12, max_rules=8, hash_seed=5)
        bes.append(b)
        b.load_snapshot(a.snapshot())  # the same table image: concurrent inserts place keys in an order of their own
        for prefixes in ([], [b"pg_03_", b"pg_5"]):
            whole = raw_scan(a, prefixes, n_cap=1 << 15, stem_cap=1 << 21)
            tiny = raw_scan(b, prefixes, n_cap=1 << 15, stem_cap=1 << 21)
            assert whole["rc"] == tiny["rc"] == abi.RL_OK and whole["raw"] == tiny["raw"] and len(whole["recs"]) > 100
            assert (whole["info"] == tiny["info"]).all() and (whole["byp"] == tiny["byp"]).all()
            n_cap = len(whole["recs"]) // 3  # (pages of about five tiles: ends inside spans of 3)
            for be in (a, b):
                cur, recs = (0, 0), []
                while cur[0] == 0:
                    res = raw_scan(be, prefixes, cur=cur, n_cap=n_cap, stem_cap=1 << 21)
                    assert res["rc"] == abi.RL_OK and res["cur"] > cur
                    recs += res["recs"]
                    cur = res["cur"]
                assert recs == whole["recs"]
    finally:
        for be in bes:
            be.close()


# --------------------------------------------------------------------------- 5. interleaving
def test_gpu_scan_with_batches_between_pages():
    """Between the pages, batches that insert new stems and hit existing ones:
    every key present before the first page comes exactly once, with the
    records of its page's moment (an export_range of the same tiles taken right
    after the page)."""
    slots = 1 << 13
    be = Backend(0.8, False, table_slots=slots, max_batch=1 << 12, max_rules=8)
    try:
        stems = paging_stems(4000)
        insert(be, stems, unit=2, now=T)
        before = {r[:2] for r in SC.export_list(be)}
        assert len(before) == 4000
        cur, seen, page, rng = (0, 0), [], 0, random.Random(3)
        while cur[0] == 0:
            res = raw_scan(be, cur=cur, n_cap=1100, stem_cap=1 << 20)  # (two tiles' worth)
            assert res["rc"] == abi.RL_OK
            end = slots if res["cur"][0] else res["cur"][1]
            rec, _ = be.export_range(0, cur[1], end)
            assert key_counts(res["recs"]) == key_counts(SC.rec_list(rec))  # (the order between keys is the export's own)
            seen += res["recs"]
            cur = res["cur"]
            page += 1
            fresh = [b"pg_new_%02d_%04d_" % (page, j) for j in range(150)]
            insert(be, fresh + rng.sample(stems, 300), unit=2, now=T + 60 * page, hits=2)
        assert page >= 4
        keys = [g[0][:2] for g in SC.groups_of(seen)]  # (asserts: no key on two pages, each key's windows in order)
        assert before <= set(keys)  # every key that was there throughout, none left out
        assert len({k for k in keys if k[0].startswith(b"pg_new_")}) < 150 * page  # (later inserts: some seen, not all)
    finally:
        be.close()


# --------------------------------------------------------------------------- 6. ordering
def test_gpu_scan_orders_after_host_batches_in_flight():
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=1 << 10, max_rules=8)
    arena = PinnedArena()
    try:
        groups = [[b"inflight_stem_%d_%03d_" % (g, j) for j in range(300)] for g in range(4)]
        keep = []
        for g, ss in enumerate(groups):
            n = len(ss)
            a = arrays_from_lists(ss, [W.NOW0 + g] * n, list(range(n)), [2] * n, [0] * n, [50] * n, [2] * n, [0] * n)
            pb = PackedBatch({k: arena.like(v) for k, v in a.items()}, n, n, 1)
            out = {k: arena.like(v) for k, v in pb.alloc_result(True).items()}
            keep.append((pb, out, be.do_limit_host_async(pb, out)))
        got, info, byp, _ = SC.scan_all(be, prefixes=[b"inflight_stem_"])  # (no synchronize before it)
        assert sorted(r[0] for r in got) == sorted(s for ss in groups for s in ss)
        assert all(r[4] == 2 for r in got) and byp == [[1200, 1200, 2400]]
        be.synchronize()
        for pb, out, _ in keep:
            assert (out["status"][:pb.n] == 0).all()
    finally:
        be.close()
        arena.close()


def test_gpu_scan_orders_after_wire_batches_in_flight():
    from ratelimit_amd.limiter import GpuRateLimitService
    from test_gpu_requests import FILES, gen_requests
    from test_gpu_wire import encode
    reqs, nows = gen_requests(4, 600)
    msgs = encode(reqs)
    svc = GpuRateLimitService(FILES, 0.8, False, "", table_slots=1 << 14, max_batch=1 << 12, max_rules=1 << 10)
    arena = PinnedArena()
    try:
        be, keep = svc.backend, []
        for lo in range(0, 600, 200):
            wb = be.wire_batch(msgs[lo:lo + 200], nows[lo:lo + 200], arena, svc._wire_rules())
            wire = {"req_status": arena.array(200, np.uint8)}
            ver = {"overall_code": arena.array(200, np.uint8)}
            keep.append((wb, wire, ver, be.do_limit_wire_async(wb, wire, None, ver)))
        first, info, _, _ = SC.scan_all(be)  # (no synchronize before it: the second halves are pending)
        be.synchronize()
        for _, w, _, _ in keep:  # (a message with a limit override is deferred to the host path: not counted here)
            assert np.isin(w["req_status"], (abi.RL_WIRE_OK, abi.RL_WIRE_DEFERRED)).all()
            assert (w["req_status"] == abi.RL_WIRE_OK).sum() > 150
        second, info2, _, _ = SC.scan_all(be)
        assert first == second and info == info2  # nothing arrived after the scan: it had waited for all three
        assert info["keys"] == be.table_info()["live_slots"] > 100
    finally:
        arena.close()
        svc.close()


# --------------------------------------------------------------------------- 7. read-only
def test_gpu_scan_changes_no_byte():
    cache, export, _ = stream_table(True, True)
    be = cache.backend
    img, info, lc = be.snapshot().tobytes(), be.table_info(), be.local_cache_info(T)
    for flags in (dict(), dict(newest=True), dict(now=T), dict(newest=True, now=T)):
        for prefixes in ((), SC.p64()):
            for kw in (dict(page_records=1 << 16), dict(page_records=64), dict(page_records=1 << 16, page_stem_bytes=600)):
                _, _, _, pages = SC.scan_all(be, prefixes=prefixes, **flags, **kw)
                assert pages >= 1
            be.count_keys(prefixes, **flags)
    assert be.snapshot().tobytes() == img and be.table_info() == info and be.local_cache_info(T) == lc
    assert key_counts(SC.export_list(be)) == key_counts(export)  # (the export's order between keys is its own)


# --------------------------------------------------------------------------- 8. shards
@pytest.mark.parametrize("n_shards", [2, 3])
def test_gpu_scan_walks_the_shards(n_shards):
    one, export, _ = stream_table(True, False)
    many, export_n, _ = stream_table(True, False, n_shards)
    assert key_counts(export) == key_counts(export_n)
    be = many.backend
    p64 = SC.p64()
    for kw in (dict(), dict(prefixes=SC.DOMAIN, now=T), dict(prefixes=p64), dict(prefixes=p64, newest=True, units=[1, 2])):
        want, winfo, wbyp = SC.expected(export, **kw)
        shards, cursors = [], []
        recs = []
        for rec, d, _ in be.scan(page_records=256, **kw):
            shards.append(d["shard"])
            cursors.append(d["cursor"])
            recs += SC.rec_list(rec)
        assert sorted(set(shards)) == list(range(n_shards)) and shards == sorted(shards)
        assert cursors == sorted(cursors) and len(set(cursors)) == len(cursors) and cursors[-1] == (n_shards, 0)
        assert all(s % TILE == 0 for _, s in cursors)
        assert key_counts(recs) == key_counts(want)
        got, ginfo, gbyp, _ = SC.scan_all(be, **kw)
        assert key_counts(got) == key_counts(want) and gbyp == wbyp
        for f, v in winfo.items():
            assert ginfo[f] == v, f
        assert ginfo["slots_scanned"] == n_shards * SMALL["table_slots"]
        cnt = be.count_keys(**kw)
        assert cnt["by_prefix"].tolist() == wbyp and cnt["slots_scanned"] == n_shards * SMALL["table_slots"]
        for f, v in winfo.items():
            assert cnt[f] == v, f
        assert one.backend.count_keys(**kw)["by_prefix"].tolist() == wbyp


# --------------------------------------------------------------------------- 9. validation
def test_gpu_scan_errors_write_nothing():
    slots = 2048
    be = Backend(0.8, False, table_slots=slots, max_batch=1 << 10, max_rules=8)
    two = Backend(0.8, False, table_slots=slots, max_batch=1 << 10, max_rules=8, n_shards=2, shard_devices=[0, 0])
    try:
        stems = paging_stems(1000)
        insert(be, stems, unit=2, now=T)
        before, info0 = SC.export_list(be), be.table_info()
        I, CAP, TIME = abi.RL_E_INVALID, abi.RL_E_CAPACITY, abi.RL_E_TIME
        NOW_MAX = (1 << 32) - 172801
        p65 = [b"q%02d_" % i for i in range(65)]
        cases = [
            (I, dict(null="q")), (I, dict(null="cur")),
            (I, dict(flags=4)), (I, dict(flags=0x80000001)),
            (I, dict(q_reserved=1)), (I, dict(cur_reserved=1)),
            (I, dict(unit_mask=1)), (I, dict(unit_mask=1 << 5)), (I, dict(unit_mask=0x80000002)),
            (I, dict(prefixes=[b"pg_", b"x"], off=np.array([1, 3, 4], np.uint32))),   # offsets do not start at 0
            (I, dict(prefixes=[b"pg_", b"x"], off=np.array([0, 3, 2], np.uint32))),   # decreasing
            (I, dict(prefixes=[b"pg_", b""])), (I, dict(prefixes=[b""])),             # an empty prefix
            (I, dict(prefixes=[b"pg_"], null="prefix_bytes")), (I, dict(prefixes=[b"pg_"], null="prefix_off")),
            (I, dict(cur=(0, 5))), (I, dict(cur=(0, TILE - 1))), (I, dict(cur=(0, slots + TILE))),
            (I, dict(cur=(0, 1 << 40))), (I, dict(cur=(2, 0))), (I, dict(cur=(1, TILE))),
            (I, dict(null="stem_off")), (I, dict(null="ws")), (I, dict(null="unit")), (I, dict(null="flags")),
            (I, dict(null="count")), (I, dict(null="expire")), (I, dict(null="lc")), (I, dict(null="stem_bytes")),
            (CAP, dict(prefixes=p65)), (CAP, dict(prefixes=[b"y" * 4097])),
            (CAP, dict(prefixes=[b"y" * 64] * 64 + [b"z"], n_prefixes=64,
                       off=np.r_[np.arange(64) * 64, 4097].astype(np.uint32))),
            (TIME, dict(flags=LIVE, now=-1)), (TIME, dict(flags=LIVE, now=NOW_MAX + 1)),
            (TIME, dict(flags=LIVE | NEWEST, now=1 << 40)),
        ]
        for want, kw in cases:
            r = raw_scan(be, **kw)
            assert r["rc"] == want and r["untouched"], kw
            if kw.get("null") not in ("stem_bytes", "stem_off") + tuple(abi.RECORD_DTYPES):
                r = raw_scan(be, out=False, **kw)  # the count-only form checks the same
                assert r["rc"] == want and r["untouched"], kw
        assert raw_scan(two, cur=(3, 0))["rc"] == I and raw_scan(two, cur=(2, TILE))["rc"] == I
        assert raw_scan(two, cur=(1, slots + TILE))["rc"] == I
        # `now` is read with RL_SCAN_LIVE only
        assert raw_scan(be, now=-1)["rc"] == abi.RL_OK and raw_scan(be, now=1 << 40, flags=NEWEST)["rc"] == abi.RL_OK
        assert raw_scan(be, flags=LIVE, now=NOW_MAX)["rc"] == abi.RL_OK
        # below the sweep floor
        be.sweep(T - 5)
        r = raw_scan(be, flags=LIVE, now=T - 6)
        assert r["rc"] == TIME and r["untouched"]
        r = raw_scan(be, flags=LIVE, now=T - 5)
        assert r["rc"] == abi.RL_OK and info_of(r)["time_floor"] == T - 5 and info_of(r)["records"] == 1000
        assert raw_scan(be, now=T - 6)["rc"] == abi.RL_OK  # (without LIVE the clock is not read)
        # a slot at the shard's end is a cursor (the last tile was covered, the API had not yet normalised it)
        r = raw_scan(be, cur=(0, slots))
        assert r["rc"] == abi.RL_OK and r["cur"] == (1, 0) and r["recs"] == [] and info_of(r)["slots_scanned"] == 0
        # a finished cursor: RL_OK and empty, on one shard and on two
        for b, done in ((be, (1, 0)), (two, (2, 0))):
            for out in (True, False):
                r = raw_scan(b, [b"pg_"], cur=done, out=out)
                assert r["rc"] == abi.RL_OK and r["cur"] == done and not r["info"].any() and not r["byp"][0].any()
                if out:
                    assert r["recs"] == [] and r["n"] == 0
        # capacities of zero: with out == NULL the call counts to the shard's end
        r = raw_scan(be, [b"pg_03_"], n_cap=0, stem_cap=0, out=False)
        want, winfo, wbyp = SC.expected(before, prefixes=[b"pg_03_"])
        i = info_of(r)
        assert r["rc"] == abi.RL_OK and r["cur"] == (1, 0) and i["slots_scanned"] == slots
        assert (i["keys"], i["records"], i["stem_bytes"]) == (winfo["keys"], winfo["records"], winfo["stem_bytes"])
        assert r["byp"][:1].tolist() == wbyp and winfo["keys"] > 0
        r = raw_scan(be, [b"pg_03_"], cur=(0, TILE), out=False)  # from the second tile on
        assert r["rc"] == abi.RL_OK and r["cur"] == (1, 0) and 0 < info_of(r)["keys"] < winfo["keys"]
        # ... and with an out of no capacity the first tile with a record is refused; empty tiles are covered
        r = raw_scan(be, [b"pg_03_"], n_cap=0, stem_cap=0)
        assert r["rc"] == CAP and info_of(r)["need_records"] > 0 and info_of(r)["need_stem_bytes"] > 0
        assert all(s.all() for s in r["sent"].values()) and r["cur"] == (0, 0) and r["n"] == 0
        r = raw_scan(be, [b"nothing_here_"], n_cap=0, stem_cap=0)
        assert r["rc"] == abi.RL_OK and r["cur"] == (1, 0) and r["n"] == 0 and info_of(r)["slots_scanned"] == slots
        # info and by_prefix are optional
        r = raw_scan(be, [b"pg_03_"], info=False, byp=False)
        assert r["rc"] == abi.RL_OK and len(r["recs"]) == winfo["records"]
        assert (r["info"] == 0xA5A5A5A5A5A5A5A5).all() and (r["byp"] == 0xA5A5A5A5A5A5A5A5).all()
        assert be.L.rl_scan(None, None, None, None, None, None) == I
        assert key_counts(SC.export_list(be)) == key_counts(before) and be.table_info() == info0
        # a ctx that joined a communicator
        from ratelimit_amd.sharded import loopback_id
        uid = loopback_id()
        be._check(be.L.rl_comm_init(be.ctx, 1, 0, abi.ptr(uid)))
        r = raw_scan(be, [b"pg_"])
        assert r["rc"] == I and r["untouched"]
    finally:
        be.close()
        two.close()


# --------------------------------------------------------------------------- the cache's call
def test_gpu_cache_list_keys_lists_a_tenants_keys():
    lim = O.new_rate_limit(5, O.MINUTE, "scan_rule")
    day = O.new_rate_limit(50, O.DAY, "scan_rule_day")
    ts = FixedTimeSource(W.NOW0)
    cache = GpuRateLimitCache(ts, 0.8, True, cache_key_prefix="p:", table_slots=1 << 10, max_batch=64, max_rules=8)
    try:
        req = O.RateLimitRequest("tenants", [O.Descriptor([("tenant", "t1")]), O.Descriptor([("tenant", "t2")])], 2)
        other = O.RateLimitRequest("tenants_b", [O.Descriptor([("tenant", "t1")])], 1)
        cache.do_limit(None, req, [lim, day])
        cache.do_limit(None, other, [lim])
        ts.now = W.NOW0 + 61  # (tenants_b's minute key, EXPIRE = NOW0 + 60, is gone)
        cache.do_limit(None, req, [lim, None])
        m0, m1, d0 = W.NOW0 // 60 * 60, (W.NOW0 + 61) // 60 * 60, W.NOW0 // 86400 * 86400
        got = sorted((k.stem, k.unit, k.ws, k.count) for k in cache.list_keys("tenants"))
        # "p:tenants_" begins the keys of "tenants" and "tenants_b", as SCAN MATCH p:tenants_* would see them;
        # tenants_b's minute window has expired by now
        assert got == [(b"p:tenants_tenant_t1_", 2, m1, 2), (b"p:tenants_tenant_t2_", 4, d0, 2)]
        every = sorted((k.stem, k.unit, k.ws, k.count) for k in cache.list_keys("tenants", live=False, newest=False))
        assert every == [(b"p:tenants_b_tenant_t1_", 2, m0, 1), (b"p:tenants_tenant_t1_", 2, m0, 2),
                         (b"p:tenants_tenant_t1_", 2, m1, 2), (b"p:tenants_tenant_t2_", 4, d0, 2)]
        only = cache.list_keys("tenants", entries=[("tenant", "t2")])
        assert [(k.stem, k.count) for k in only] == [(b"p:tenants_tenant_t2_", 2)]
        assert cache.list_keys("nobody") == []
    finally:
        cache.close()
