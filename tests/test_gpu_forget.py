"""rl_forget on the GPU: deletion of stems by key and by prefix (Redis DEL;
Backend.forget, GpuRateLimitCache.forget / forget_domain).

The expected state comes from the Python oracle, whose stores are plain dicts:
the same deletion is applied to it by removing every key k of client.data,
per_second_client.data and local_cache.data with k.rstrip("0123456789") equal
to the stem (prefix mode: beginning with the prefix), which is exact because
every stem ends in "_". The stream below gives the deletion something of every
kind to remove: stems under two units, stems longer than the slot's inline
bytes, stems the local cache blocks at the deletion's clock, stems with a
history chain; test_forget_stream_has_every_case shows that with the oracle
alone, on the CPU.
"""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import c_oracle
from oracle import oracle as O
from ratelimit_amd import abi, workloads as W
from ratelimit_amd.limiter import Backend, FixedTimeSource, GpuRateLimitCache, PinnedArena
from ratelimit_amd.packing import PackedBatch, arrays_from_lists, stem_of
import streams

gpu = pytest.mark.gpu

DIV = {1: 1, 2: 60, 3: 3600, 4: 86400}
SMALL = dict(table_slots=1 << 14, max_batch=1 << 12, max_rules=1 << 10)
NEVER = b"fg_stem_never_seen_"


# --------------------------------------------------------------------------- the stream and the oracle's deletion
def fg_stream(seed, n_calls=2400, n_stems=48):
    """Zipf-skewed stems of the domains "fg" and "fg_b", one unit each (SECOND,
    MINUTE, DAY) but for every sixth, which is also counted under HOUR; every
    fifth stem is longer than 36 bytes; small limits, hits 1..4, a
    non-decreasing clock that mostly stands, often steps one second (SECOND
    keys get history chains) and crosses minutes."""
    rng = random.Random(seed)
    reg = {}

    def rule(s, unit):
        if (s % 7, unit) not in reg:
            reg[(s % 7, unit)] = O.new_rate_limit(5 + 3 * (s % 7), unit, "fg_rule%d_u%d" % (s % 7, unit),
                                                  shadow_mode=(s % 11 == 0 and unit != O.HOUR))
        return reg[(s % 7, unit)]

    def entries(s):
        e = [("stem", "s%03d" % s)]
        if s % 5 == 2:
            e.append(("path", "/a/rather/long/path/component/%03d" % s))
        return e

    w = [1.0 / (i + 1) ** 1.1 for i in range(n_stems)]
    units = [(O.SECOND, O.MINUTE, O.MINUTE, O.SECOND, O.DAY, O.MINUTE)[s % 6] for s in range(n_stems)]
    calls, now = [], 1_700_000_030
    for _ in range(n_calls):
        now += rng.choice([0] * 60 + [1, 1, 1, 2, 20])
        per_dom = {}
        for _d in range(rng.randint(1, 3)):
            s = rng.choices(range(n_stems), w)[0]
            unit = O.HOUR if s % 6 == 1 and rng.random() < 0.3 else units[s]
            d, l = per_dom.setdefault("fg" if s % 3 else "fg_b", ([], []))
            d.append(O.Descriptor(entries(s)))
            l.append(rule(s, unit))
        for dom, (d, l) in per_dom.items():
            calls.append((O.RateLimitRequest(dom, d, rng.randint(1, 4)), l, now))
    return calls


def oracle_forget(oc, stems=(), prefixes=()):
    """DEL of every key of the stems (or under the prefixes) in the oracle's
    stores and its freecache. -> keys deleted."""
    stems = {s.decode() for s in stems}
    prefixes = [p.decode() for p in prefixes]
    n = 0
    for store in (oc.client, oc.per_second_client, oc.local_cache):
        if store is None:
            continue
        for k in list(store.data):
            s = k.rstrip("0123456789")
            if s in stems or any(s.startswith(p) for p in prefixes):
                del store.data[k]
                n += 1
    return n


def seen_keys(calls):
    """{stem: {unit: set of window starts}} of the calls' non-nil descriptors."""
    seen = {}
    for r, l, now in calls:
        for d, lim in zip(r.descriptors, l):
            if lim is not None:
                u = lim.limit.unit
                seen.setdefault(stem_of("", r.domain, d.entries), {}).setdefault(u, set()).add(now // DIV[u] * DIV[u])
    return seen


def plan(calls, half, local_cache, per_second):
    """The oracle after calls[:half], the deletion's clock, and the stems to
    forget with the kinds among them: asserts that each kind is there."""
    oc = O.OracleFixedRateLimitCache(0.8, local_cache, per_second=per_second)
    for r, l, now in calls[:half]:
        oc.do_limit(r, l, now)
    T = calls[half][2]
    assert all(a[2] <= b[2] for a, b in zip(calls, calls[1:]))  # non-decreasing clocks
    seen = seen_keys(calls[:half])
    later = seen_keys(calls[half:])
    kinds = {
        "two_units": [s for s in seen if len(seen[s]) >= 2],
        "long": [s for s in seen if len(s) > 36],
        # a slot has a chain once its newest window moved while the older one was within 8 windows of it
        "history": [s for s in seen for u, ws in seen[s].items()
                    if any(0 < a - b <= 8 * DIV[u] for a in ws for b in ws)],
        "blocked": [s for s in seen if local_cache and any(
            k.rstrip("0123456789") == s.decode() and e > T for k, e in oc.local_cache.data.items())],
    }
    chosen = []
    for kind, lst in kinds.items():
        if kind == "blocked" and not local_cache:
            continue
        hit_again = [s for s in lst if s in later]  # (the second half must meet the deletion)
        assert len(hit_again) >= 2, (kind, len(lst))
        chosen += [s for s in hit_again[:3] if s not in chosen]
    chosen += [s for s in sorted(seen)[::5] if s not in chosen]
    chosen.append(NEVER)
    assert NEVER not in seen and len(chosen) < len(seen) // 2  # (most stems stay)
    return oc, T, chosen, seen, kinds


def st(s):
    cl = None if s.current_limit is None else (s.current_limit.requests_per_unit, s.current_limit.unit)
    return (s.code, cl, s.limit_remaining, s.duration_until_reset)


def stats_of(calls):
    return {l.stats.key: l.stats.as_tuple() for _, ls, _ in calls for l in ls if l is not None}


def run_gpu(cache, calls, chunk=400):
    out = []  # (do_limit_batch raises unless every descriptor's status is RL_OK)
    for i in range(0, len(calls), chunk):
        out += cache.do_limit_batch(calls[i:i + chunk])
    return out


def arena_bytes(stem):
    return (len(stem) - 32 + 15) // 16 * 16 if len(stem) > 36 else 0


def export_all(be):
    """[(stem, unit, flags, ws, count, expire, lc)] of the whole table, sorted."""
    recs = []
    for part in be.export_records():
        off, sb = part["stem_off"], part["stem_bytes"]
        recs += [(bytes(sb[off[i]:off[i + 1]]),) + tuple(int(part[k][i]) for k in abi.RECORD_DTYPES)
                 for i in range(len(part["ws"]))]
    return sorted(recs)


@pytest.mark.parametrize("local_cache,per_second", [(True, False), (False, True)])
def test_forget_stream_has_every_case(local_cache, per_second):
    """CPU, the oracle alone: the stream's first half holds stems under two
    units, long stems, stems with two windows within the history's reach and
    (with the local cache) stems blocked at the deletion's clock, each hit again
    afterwards; and deleting them changes what the oracle answers."""
    calls = fg_stream(5)
    half = len(calls) // 2
    oc, T, chosen, seen, kinds = plan(calls, half, local_cache, per_second)
    assert any(len(seen[s]) >= 2 for s in chosen) and any(len(s) > 36 for s in chosen)
    assert any(s in kinds["history"] for s in chosen)
    if local_cache:
        assert any(s in kinds["blocked"] for s in chosen)
    assert oracle_forget(oc, chosen) > len(chosen) // 2
    plain = O.OracleFixedRateLimitCache(0.8, local_cache, per_second=per_second)
    for r, l, now in calls[:half]:
        plain.do_limit(r, l, now)
    a = [[st(s) for s in oc.do_limit(r, l, now)] for r, l, now in calls[half:]]
    b = [[st(s) for s in plain.do_limit(r, l, now)] for r, l, now in calls[half:]]
    assert sum(x != y for x, y in zip(a, b)) > 20  # (a test that skipped the deletion would fail)


# --------------------------------------------------------------------------- 1. parity across a deletion
@gpu
@pytest.mark.parametrize("per_second", [False, True])
@pytest.mark.parametrize("local_cache", [False, True])
def test_gpu_forget_parity_across_a_deletion(local_cache, per_second):
    """Half the stream, forget the chosen stems, the rest: every code,
    remaining, reset and per-rule stats delta of the second half is the
    oracle's after the same deletion (do_limit_batch raises unless every
    descriptor's status is RL_OK; none is left out)."""
    calls = fg_stream(5)
    half = len(calls) // 2
    oc, T, chosen, seen, kinds = plan(calls, half, local_cache, per_second)
    cache = GpuRateLimitCache(FixedTimeSource(0), 0.8, local_cache, per_second=per_second, **SMALL)
    try:
        run_gpu(cache, calls[:half])
        got = cache.backend.forget(chosen)
        want_removed = [len(seen.get(s, ())) for s in chosen]
        assert got["removed"].tolist() == want_removed
        assert max(want_removed) >= 2 and want_removed[-1] == 0  # two units; the stem never seen
        assert got["keys"] == sum(want_removed) and got["slots_scanned"] == 0
        assert got["keys_with_history"] > 0
        assert got["arena_bytes"] == sum(arena_bytes(s) * len(seen.get(s, ())) for s in chosen) > 0
        oracle_forget(oc, chosen)
        streams.reset_stats(calls)
        want = [[st(s) for s in oc.do_limit(r, l, now)] for r, l, now in calls[half:]]
        want_stats = stats_of(calls)
        streams.reset_stats(calls)
        out = [[st(s) for s in g] for g in run_gpu(cache, calls[half:])]
        assert len(out) == len(want)
        bad = [i for i, (g, w) in enumerate(zip(out, want)) if g != w]
        assert not bad, (len(bad), bad[:3], out[bad[0]], want[bad[0]])
        assert stats_of(calls) == want_stats
    finally:
        cache.close()


# --------------------------------------------------------------------------- 2. reads after deletion
@gpu
def test_gpu_forget_reads_after_deletion():
    """After the deletion at T: rl_lookup of every removed (stem, unit) is not
    found, count 0, lc 0; the export holds every other key's records unchanged
    and none of a removed stem; table_info and the local-cache entry count move
    as specified."""
    calls = fg_stream(5)
    half = len(calls) // 2
    oc, T, chosen, seen, _ = plan(calls, half, True, False)
    cache = GpuRateLimitCache(FixedTimeSource(0), 0.8, True, **SMALL)
    be = cache.backend
    try:
        run_gpu(cache, calls[:half])
        before, info0 = export_all(be), be.table_info()
        assert be.local_cache_info(T)["entry_count"] == oc.local_cache.entry_count(T) > 0
        got = be.forget(chosen)
        after, info1 = export_all(be), be.table_info()
        gone = set(chosen)
        assert after == [r for r in before if r[0] not in gone]
        assert len(before) - len(after) >= got["keys"] > 0
        keys = [(s, u) for s in chosen for u in sorted(seen.get(s, ()))]
        res = be.lookup([k[0] for k in keys], [k[1] for k in keys], [T] * len(keys))
        for f in ("status", "found", "count", "expire", "lc"):
            assert not res[f].any(), f
        exact = sum(n for n in got["removed"].tolist() if n >= 2)
        assert exact > 0 and got["keys_with_history"] > 0
        moved = {"live_slots": -got["keys"], "tombstones": got["keys"], "exact_stems": -exact,
                 "history_slots": -got["keys_with_history"]}
        for f, v in info0.items():
            assert info1[f] == v + moved.get(f, 0), f  # (history_*, batches, decisions, the arena's cursor: as before)
        oracle_forget(oc, chosen)
        assert be.local_cache_info(T)["entry_count"] == oc.local_cache.entry_count(T)
        # the arena's bytes come back at the next sweep's compaction, even one that evicts nothing
        be.sweep(T)
        info2 = be.table_info()
        assert info0["arena_bytes_used"] - info2["arena_bytes_used"] >= got["arena_bytes"] > 0
    finally:
        cache.close()


# --------------------------------------------------------------------------- 3. prefix mode at the layout's edges
BASE = b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ" * 4
EDGE_LEN = (4, 5, 31, 32, 33, 36, 37, 48, 49, 200)


def edge_stems():
    """Stems of the edge lengths sharing their beginnings: BASE cut at L; the
    same with its last byte changed; with byte 33 changed (the arena's second
    byte, or inline byte 33); and a family that differs in the first byte."""
    out = set()
    for L in EDGE_LEN:
        s = BASE[:L]
        out |= {s, s[:-1] + b"#", b"X" + s[1:]}
        if L > 34:
            out.add(s[:33] + b"#" + s[34:])
    return sorted(out)


PREFIX_CASES = [[BASE[:k]] for k in (1, 4, 5, 31, 32, 33, 36, 37, 40)] + [
    [BASE[:33], BASE[:5]],          # one begins the other: counted under the lower index
    [BASE[:5], BASE[:33]],          # (the longer one then counts nothing)
    [BASE[:36] + b"?", BASE[:48], b"Xbcd", BASE[:31] + b"#"],
]


def insert(be, stems, unit=2, now=W.NOW0, hits=1, limit=1000):
    n = len(stems)
    a = arrays_from_lists(stems, [now] * n, list(range(n)), [unit] * n, [0] * n, [limit] * n, [hits] * n, [0] * n)
    g = be.do_limit_arrays(a, n, n, 1, isolate=True)
    assert (g["status"] == 0).all()
    return g


@gpu
def test_gpu_forget_prefixes_at_the_layout_edges():
    stems = edge_stems()
    assert BASE[:36] in stems and len(stems) > 30
    for prefixes in PREFIX_CASES:
        be = Backend(0.8, False, table_slots=1 << 10, max_batch=1 << 10, max_rules=8)
        try:
            insert(be, stems)
            assert sorted({r[0] for r in export_all(be)}) == stems
            want = [0] * len(prefixes)
            for s in stems:  # Python's startswith over the exported stems, the lowest matching index
                hit = [i for i, p in enumerate(prefixes) if s.startswith(p)]
                if hit:
                    want[hit[0]] += 1
            dry = be.forget(prefixes, prefix=True, dry_run=True)
            got = be.forget(prefixes, prefix=True)
            assert got["removed"].tolist() == want == dry["removed"].tolist(), prefixes
            assert sum(want) > 0 and got["keys"] == sum(want) and got["slots_scanned"] == 1 << 10
            assert got["arena_bytes"] == sum(arena_bytes(s) for s in stems if any(s.startswith(p) for p in prefixes))
            assert sorted({r[0] for r in export_all(be)}) == [s for s in stems if not any(s.startswith(p) for p in prefixes)]
        finally:
            be.close()


@gpu
def test_gpu_forget_prefix_capacity():
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=1 << 10, max_rules=8)
    try:
        fam = [b"%02d" % j * 32 + b"_tail_%d_" % j for j in range(70)]  # 64 bytes of j's digits, then a tail
        insert(be, fam)
        before = export_all(be)
        p64 = [s[:64] for s in fam[:64]]
        assert sum(map(len, p64)) == 4096
        for bad in ([s[:64] for s in fam[:65]], p64[:63] + [fam[63][:65]], [b"y" * 4097]):
            s = raw(be, bad, abi.RL_FORGET_PREFIX)
            assert s[0] == abi.RL_E_CAPACITY and untouched(s), len(bad)
            assert export_all(be) == before
        got = be.forget(p64, prefix=True)
        assert got["removed"].tolist() == [1] * 64 and got["keys"] == 64
        assert sorted({r[0] for r in export_all(be)}) == sorted(fam[64:])
    finally:
        be.close()


# --------------------------------------------------------------------------- 4. dry run
@gpu
def test_gpu_forget_dry_run_changes_nothing_and_tells_the_same():
    calls = fg_stream(5)
    half = len(calls) // 2
    _, T, chosen, seen, _ = plan(calls, half, True, False)
    cache = GpuRateLimitCache(FixedTimeSource(0), 0.8, True, **SMALL)
    be = cache.backend
    try:
        run_gpu(cache, calls[:half])
        for kw in (dict(stems=chosen), dict(stems=[b"fg_b_"], prefix=True)):
            before, info0, lc0 = export_all(be), be.table_info(), be.local_cache_info(T)
            dry = be.forget(dry_run=True, **kw)
            assert export_all(be) == before and be.table_info() == info0 and be.local_cache_info(T) == lc0
            real = be.forget(**kw)
            assert dry["removed"].tolist() == real["removed"].tolist()
            assert {k: v for k, v in dry.items() if k != "removed"} == {k: v for k, v in real.items() if k != "removed"}
            assert real["keys"] > 0
            assert be.forget(dry_run=True, **kw)["keys"] == 0  # (nothing is left to remove)
        left = {r[0] for r in export_all(be)}
        assert left and not any(s.startswith(b"fg_b_") for s in left)  # (the domain "fg" stays)
        assert cache.forget_domain("fg", dry_run=True)["keys"] == be.table_info()["live_slots"]
    finally:
        cache.close()


# --------------------------------------------------------------------------- 5. duplicates
@gpu
@pytest.mark.parametrize("dry_run", [False, True])
def test_gpu_forget_counts_a_stem_listed_three_times_once(dry_run):
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=1 << 10, max_rules=8)
    try:
        long = b"dup_stem_long_" + b"z" * 60 + b"_"
        for unit in (1, 2, 4):
            insert(be, [b"dup_stem_", long, b"other_stem_"], unit=unit)
        stems = [b"dup_stem_", long, b"dup_stem_", b"absent_stem_", long, b"dup_stem_", long] * 40  # many lanes, one workgroup and more
        got = be.forget(stems, dry_run=dry_run)
        assert int(got["removed"].sum()) == got["keys"] == 6
        assert got["arena_bytes"] == 3 * arena_bytes(long)
        idx = {s: [i for i, x in enumerate(stems) if x == s] for s in set(stems)}
        assert int(got["removed"][idx[b"dup_stem_"]].sum()) == 3 == int(got["removed"][idx[long]].sum())
        assert be.table_info()["live_slots"] == (9 if dry_run else 3)
    finally:
        be.close()


# --------------------------------------------------------------------------- 6. probe paths
@gpu
def test_gpu_forget_keeps_probe_paths():
    """debug_hash_bits=2: four home slots, so every key lies on a long run and
    the forgotten keys lie between other keys' homes and slots. The survivors
    are still found and answered like the C oracle's (which never saw the
    forgotten keys: keys are independent), and the forgotten stems insert again."""
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=1 << 10, max_rules=8, debug_hash_bits=2, hash_seed=9)
    co = c_oracle.COracle(0.8, False)
    try:
        stems = [b"crowded_stem_%04d_%s" % (j, b"x" * (j % 50)) for j in range(600)]
        T = W.NOW0
        order = sorted(range(600), key=lambda j: (j * 7919) % 600)
        gone, keep = [stems[j] for j in order if j % 3 == 0], [stems[j] for j in order if j % 3]

        def batch(ss, now, hits):
            n = len(ss)
            return arrays_from_lists(ss, [now] * n, list(range(n)), [2] * n, [0] * n, [1000] * n, hits, [0] * n), n, n, 1

        for lo in range(0, 600, 200):  # interleaved: the forgotten keys lie on the paths of the kept ones
            part = [stems[j] for j in order[lo:lo + 200]]
            be.do_limit_arrays(*batch(part, T, [1 + len(s) % 5 for s in part]), isolate=True)
        kb = batch(keep, T, [1 + len(s) % 5 for s in keep])
        co.do_limit(*kb)
        got = be.forget(gone)
        assert got["removed"].tolist() == [1] * 200
        info = be.table_info()
        assert info["live_slots"] == 400 and info["tombstones"] == 200
        res = be.lookup(keep + gone, [2] * 600, [T + 1] * 600)
        assert (res["status"] == 0).all() and res["found"][:400].all() and not res["found"][400:].any()
        assert res["count"][:400].tolist() == [1 + len(s) % 5 for s in keep]
        for b in (batch(keep, T + 2, [2] * 400), batch(gone, T + 3, [3] * 200), batch(stems, T + 4, [1] * 600)):
            g, o = be.do_limit_arrays(*b, isolate=True), co.do_limit(*b)
            assert (g["status"] == 0).all()
            for k in ("code", "limit_remaining", "reset_s", "stats"):
                assert np.array_equal(g[k], o[k]), k
        assert be.table_info()["live_slots"] == 600
    finally:
        be.close()
        co.close()


@gpu
def test_gpu_forgotten_slots_are_reclaimed_by_the_sweep():
    """The sweep's existing rule: on a table left with less than a quarter of
    its slots empty the tombstones no live key needs become empty again.
    Forgotten slots take part like swept ones."""
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=1 << 10, max_rules=8, hash_seed=3)
    try:
        first = [b"reclaim_stem_%04d_" % j for j in range(900)]
        insert(be, first, now=W.NOW0)
        assert be.forget(first[:600])["keys"] == 600
        info = be.table_info()
        assert info["tombstones"] == 600 and info["live_slots"] == 300  # 124 slots empty: less than a quarter
        assert be.sweep(W.NOW0 + 1) == 0  # (nothing expires: the tombstones are the deletion's)
        info = be.table_info()
        assert info["live_slots"] == 300 and info["tombstones"] < 600
        fresh = [b"fresh_stem_%04d_" % j for j in range(700)]
        insert(be, fresh, now=W.NOW0 + 2)
        res = be.lookup(first[600:] + fresh, [2] * 1000, [W.NOW0 + 2] * 1000)
        assert res["found"].all() and be.table_info()["live_slots"] == 1000
    finally:
        be.close()


# --------------------------------------------------------------------------- 7. shards
@gpu
def test_gpu_forget_on_two_shards_equals_one():
    calls = fg_stream(5)
    half = len(calls) // 2
    _, T, chosen, seen, _ = plan(calls, half, True, False)
    one = GpuRateLimitCache(FixedTimeSource(0), 0.8, True, **SMALL)
    two = GpuRateLimitCache(FixedTimeSource(0), 0.8, True, n_shards=2, shard_devices=[0, 0], **SMALL)
    try:
        for c in (one, two):
            run_gpu(c, calls[:half])
        assert export_all(one.backend) == export_all(two.backend)
        prefixes = [b"fg_b_stem_s00", b"fg_stem_s01", b"fg_b_"]
        for kw in (dict(stems=chosen, dry_run=True), dict(stems=chosen), dict(stems=prefixes, prefix=True, dry_run=True),
                   dict(stems=prefixes, prefix=True)):
            a, b = one.backend.forget(**kw), two.backend.forget(**kw)
            assert a["removed"].tolist() == b["removed"].tolist() and a["keys"] > 0, kw
            assert b["slots_scanned"] == 2 * a["slots_scanned"] == (2 << 14 if kw.get("prefix") else 0)
            for f in ("keys", "keys_with_history", "arena_bytes"):
                assert a[f] == b[f], f
            assert export_all(one.backend) == export_all(two.backend)
        out = [[[st(s) for s in g] for g in run_gpu(c, calls[half:])] for c in (one, two)]
        assert out[0] == out[1]
    finally:
        one.close()
        two.close()


# --------------------------------------------------------------------------- 8. ordering and persistence
@gpu
def test_gpu_forget_orders_after_batches_in_flight():
    """Host-fed batches submitted without waiting, the deletion at once: it sees
    their keys, and the batch after it counts them from zero."""
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
        got = be.forget(groups[3] + groups[0])  # (no synchronize before it)
        assert got["removed"].tolist() == [1] * 600
        be.synchronize()
        for pb, out, _ in keep:
            assert (out["status"][:pb.n] == 0).all() and (out["limit_remaining"][:pb.n] == 48).all()
        g = insert(be, groups[0] + groups[1], now=W.NOW0 + 5, hits=3, limit=50)
        assert g["limit_remaining"].tolist() == [47] * 300 + [45] * 300
    finally:
        be.close()
        arena.close()


@gpu
def test_gpu_forget_then_snapshot_replays_like_the_original():
    calls = fg_stream(5)
    half = len(calls) // 2
    oc, T, chosen, _, _ = plan(calls, half, True, False)
    a = GpuRateLimitCache(FixedTimeSource(0), 0.8, True, **SMALL)
    b = GpuRateLimitCache(FixedTimeSource(0), 0.8, True, **SMALL)
    try:
        run_gpu(a, calls[:half])
        a.backend.forget(chosen)
        assert a.forget_domain("fg_b")["keys"] > 0
        img = a.backend.snapshot()
        b.backend.load_snapshot(img)
        assert export_all(a.backend) == export_all(b.backend)
        oracle_forget(oc, chosen, [b"fg_b_"])
        want = [[st(s) for s in oc.do_limit(r, l, now)] for r, l, now in calls[half:]]
        b.interner = a.interner  # (the same rule ids: the snapshot holds no rule table)
        for c in (a, b):
            assert [[st(s) for s in g] for g in run_gpu(c, calls[half:])] == want
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------- 9. errors
SENT = 0xA5A5A5A5


def raw(be, stems, flags=0, n=None, off=None, blob=None, null=None, info=True):
    """rl_forget as a C caller makes it, the outputs pre-filled with a sentinel:
    -> (rc, removed, info words)."""
    m = len(stems) if n is None else n
    if off is None:
        off = np.r_[0, np.cumsum([len(s) for s in stems])].astype(np.uint32)
    if blob is None:
        blob = np.frombuffer(b"".join(stems) or b"\0", np.uint8).copy()
    removed = np.full(max(m, 1) + 4, SENT, np.uint32)
    words = np.full(4, SENT, np.uint64)
    s = abi.RlStems()
    s.n, s.flags = m, flags
    s.stem_bytes = None if null == "stem_bytes" else abi.ptr(blob)
    s.stem_off = None if null == "stem_off" else abi.ptr(off)
    rc = be.L.rl_forget(be.ctx, None if null == "in" else C.byref(s), abi.ptr(removed),
                        C.cast(abi.ptr(words), C.POINTER(abi.RlForgetInfo)) if info else None)
    return rc, removed, words


def untouched(r):
    return (r[1] == SENT).all() and (r[2] == SENT).all()


@gpu
def test_gpu_forget_errors_change_nothing():
    MB = 256
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=MB, max_rules=8, max_stem_bytes=1 << 14)
    try:
        stems = [b"error_stem_%04d_" % j for j in range(MB + 1)]
        insert(be, stems[:200])
        before, info0 = export_all(be), be.table_info()
        I, CAP = abi.RL_E_INVALID, abi.RL_E_CAPACITY
        P = abi.RL_FORGET_PREFIX
        cases = [
            (I, dict(stems=stems[:3], null="in")), (I, dict(stems=stems[:3], null="stem_bytes")),
            (I, dict(stems=stems[:3], null="stem_off")),
            (I, dict(stems=[], n=2, off=np.array([1, 4, 8], np.uint32), blob=np.zeros(16, np.uint8))),
            (I, dict(stems=[], n=2, off=np.array([0, 8, 4], np.uint32), blob=np.zeros(16, np.uint8))),
            (I, dict(stems=[stems[0], b"", stems[1]])),                 # an empty stem
            (I, dict(stems=[b"error_", b""], flags=P)),                 # an empty prefix: no "flush everything"
            (I, dict(stems=[b""], flags=P | abi.RL_FORGET_DRY_RUN)),
            (I, dict(stems=stems[:3], flags=4)), (I, dict(stems=stems[:3], flags=0x80000001)),
            (I, dict(stems=[b"e" * 65536])),                            # over 65535 bytes
            (CAP, dict(stems=stems[:MB + 1])),                          # n > max_batch
            (CAP, dict(stems=[b"e" * 9000] * 2)),                       # stem bytes > max_stem_bytes
        ]
        for want, kw in cases:
            r = raw(be, **kw)
            assert r[0] == want and untouched(r), kw.get("null") or kw.get("flags") or len(kw["stems"])
        assert be.L.rl_forget(be.ctx, None, None, None) == I
        assert export_all(be) == before and be.table_info() == info0
        # n == 0 is RL_OK (either mode; null arrays are fine then), *info zero, removed untouched
        for flags in (0, P):
            rc, removed, words = raw(be, [], flags, null="stem_off")
            assert rc == abi.RL_OK and (removed == SENT).all() and not words.any()
        # removed and info are optional; entries past n are not written
        s = abi.RlStems()
        blob = np.frombuffer(stems[0], np.uint8).copy()
        off = np.array([0, len(stems[0])], np.uint32)
        s.n, s.flags, s.stem_bytes, s.stem_off = 1, 0, abi.ptr(blob), abi.ptr(off)
        assert be.L.rl_forget(be.ctx, C.byref(s), None, None) == abi.RL_OK
        rc, removed, words = raw(be, stems[:MB])
        assert rc == abi.RL_OK and removed[:MB].tolist() == [0] + [1] * 199 + [0] * (MB - 200)
        assert (removed[MB:] == SENT).all() and words.tolist() == [0, 199, 0, 0]
        # a ctx that joined a communicator
        from ratelimit_amd.sharded import loopback_id
        uid = loopback_id()
        be._check(be.L.rl_comm_init(be.ctx, 1, 0, abi.ptr(uid)))
        r = raw(be, stems[:3])
        assert r[0] == I and untouched(r)
    finally:
        be.close()


# --------------------------------------------------------------------------- the cache's calls
@gpu
def test_gpu_cache_forget_unblocks_a_tenant():
    """The operator's case: a DAY key blocked in the local over-limit cache is
    let through at once, under a cache key prefix."""
    lim = O.new_rate_limit(3, O.DAY, "forget_rule")
    req = O.RateLimitRequest("tenants", [O.Descriptor([("tenant", "t1")]), O.Descriptor([("nil", "x")])], 2)
    other = O.RateLimitRequest("tenants_b", [O.Descriptor([("tenant", "t1")])], 2)
    cache = GpuRateLimitCache(FixedTimeSource(W.NOW0), 0.8, True, cache_key_prefix="p:", table_slots=1 << 10,
                              max_batch=64, max_rules=8)
    try:
        for _ in range(3):
            cache.do_limit(None, req, [lim, None])
            cache.do_limit(None, other, [lim])
        assert cache.peek(req, [lim, None])[0].over_limit_cached
        assert cache.do_limit(None, req, [lim, None])[0].code == O.OVER_LIMIT
        assert cache.forget(req, [lim, None], dry_run=True)["removed"].tolist() == [1]
        assert cache.forget(req, [lim, None])["removed"].tolist() == [1]
        assert cache.peek(req, [lim, None])[0] == (0, None, False)
        s = cache.do_limit(None, req, [lim, None])[0]
        assert s.code == O.OK and s.limit_remaining == 1
        assert cache.do_limit(None, other, [lim])[0].code == O.OVER_LIMIT  # (another domain's key stays)
        # "p:tenants_" begins the keys of the domains "tenants" and "tenants_b", as SCAN MATCH p:tenants_* would
        assert cache.forget_domain("tenants")["keys"] == 2
        assert cache.backend.table_info()["live_slots"] == 0
    finally:
        cache.close()
