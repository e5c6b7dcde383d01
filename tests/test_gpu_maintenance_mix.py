"""The maintenance calls in combination, on the GPU: rl_forget (keyed and by
prefix), rl_sweep, rl_resize, rl_resize_history, rl_resize_arena, snapshot
save / load and limiter.migrate, one after another on one ctx.

Each of those calls has a test file of its own that runs a stream, makes one
call and continues. Here one stream runs against one Python oracle through four
walks of 26 calls, ordered so that every ordered pair of calls occurs back to
back once (tests/maintenance_mix.py; tests/test_maintenance_mix_cpu.py proves
the plan with the oracle alone: every pair, every step felt by the calls after
it, every checker able to fail). After every call every reader of the table
(export, scan, hot keys, lookup, table info, the local-cache gauge) is compared
with the oracle, and the call's own info with the exports around it; after
every segment of the stream every code, remaining, reset and stats delta is
the oracle's. The walks lose no history by themselves (asserted from
history_appended), so no descriptor is left out of any comparison.
"""
import pytest

from ratelimit_amd import abi, workloads as W
from ratelimit_amd.limiter import Backend, FixedTimeSource, GpuRateLimitCache, migrate
from ratelimit_amd.packing import arrays_from_lists
import maintenance_mix as M
import scan_cases as SC
import streams
from test_gpu_forget import insert, run_gpu, st, stats_of

pytestmark = pytest.mark.gpu


def _fresh(be, **over):
    """A new Backend of be's current geometry (its rl_config as the resizes left it), but for `over`."""
    c = be.cfg
    kw = dict(table_slots=int(c.table_slots), max_batch=int(c.max_batch), max_rules=int(c.max_rules),
              device=int(c.device), arena_bytes=int(c.arena_bytes), max_stem_bytes=int(c.max_stem_bytes),
              hash_seed=int(c.hash_seed), debug_hash_bits=int(c.debug_hash_bits), n_shards=be.n_shards(),
              history_entries=int(c.history_entries))
    kw.update(over)
    kw["shard_devices"] = [int(c.device)] * kw["n_shards"]
    return Backend(float(c.near_limit_ratio), bool(c.local_cache_enabled), bool(c.per_second_split),
                   int(c.expiration_jitter_max_seconds), **kw)


def _call(cache, op, a):
    """Step `op` on the cache's backend -> (the call's info, history_appended of a ctx it closed)."""
    be = cache.backend
    if op in ("F_KEYS", "F_PREFIX"):
        return be.forget(a, prefix=op == "F_PREFIX"), 0
    if op == "SWEEP":
        return be.sweep(a), 0
    if op in ("T_SMALL", "T_LARGE"):
        return be.resize(a), 0  # (raises unless every key was placed)
    if op in ("H_SMALL", "H_LARGE"):
        return be.resize_history(a), 0
    if op == "ARENA":
        return be.resize_arena(a), 0
    new = _fresh(be, **(a if op == "MIGRATE" else {}))
    try:
        if op == "SNAPSHOT":
            new.load_snapshot(be.snapshot())
            got = None
        else:
            got = migrate(be, new)
    except BaseException:
        new.close()
        raise
    appended = be.table_info()["history_appended"]
    be.close()
    cache.backend = new
    return got, appended


def _segment(cache, wk, i, where):
    calls = wk.segments[i]
    want, want_stats = wk.segment(i)
    streams.reset_stats(calls)
    out = [[st(s) for s in g] for g in run_gpu(cache, calls)]  # (raises unless every status is RL_OK)
    diff = M.first_difference(out, want, calls)
    assert diff is None, "%s, segment %d: first differing descriptor %r" % (where, i, diff)
    assert stats_of(calls) == want_stats, "%s, segment %d: the per-rule stats differ" % (where, i)


@pytest.mark.parametrize("walk", range(4))
def test_gpu_maintenance_mix_walk(walk):
    wk = M.Walk(walk)
    kw = dict(M.CTX, debug_hash_bits=wk.hash_bits)
    if wk.shards > 1:
        kw.update(n_shards=wk.shards, shard_devices=[0] * wk.shards)
    cache = GpuRateLimitCache(FixedTimeSource(0), 0.8, wk.lc, cache_key_prefix=wk.prefix, per_second=wk.per_second,
                              **kw)
    appended, where = 0, "walk %d, before step 0" % walk
    try:
        _segment(cache, wk, 0, where)
        for i, op in enumerate(wk.ops):
            where = "walk %d, step %d, pair (%s, %s)" % (walk, i, wk.ops[i - 1] if i else None, op)
            try:
                rd = M.GpuReader(cache.backend)
                pre, ia = rd.export(), rd.table_info()
                a, tomb_zero = wk.args(i), wk.tomb_zero
                got, closed = _call(cache, op, a)
                appended += closed
                wk.apply(i, a)
                if op == "SWEEP":  # (the sweep's own count says whether it left tombstones)
                    wk.tomb_zero = tomb_zero and got == 0
                rd = M.GpuReader(cache.backend)
                ib = rd.table_info()
                # arena_bytes_used: the live long stems' bytes after a sweep's compaction, unchanged by every
                # other call on the same ctx or its image, bounded below after an import
                exact = "live" if op == "SWEEP" else None if op == "MIGRATE" else ia["arena_bytes_used"]
                post = M.check_readers(rd, wk, exact)
                M.check_op(op, a, got, pre, ia, post, ib, wk)
                if isinstance(got, dict):
                    got = {k: v for k, v in got.items() if k != "removed"}
                print(where, a if op not in ("F_KEYS", "F_PREFIX") else len(a), got, "keys", ib["live_slots"],
                      "records", len(post), "tombstones", ib["tombstones"], "appended", ib["history_appended"])
            except AssertionError as e:
                raise AssertionError("%s: %s" % (where, e)) from e
            _segment(cache, wk, i + 1, where)
        info = cache.backend.table_info()
        appended += info["history_appended"]
        print("walk %d: history_appended over its ctxs %d of %d, late calls that read a window from before the "
              "step %d, calls %d" % (walk, appended, M.H_FLOOR // 64, wk.late_reads, wk.tick))
        # no partition can have wrapped or refused, had every append fallen into one: the walk lost no history itself
        assert appended < M.H_FLOOR // 64
        assert info["history_lost"] == 0 and info["history_refused"] == 0
    finally:
        cache.backend.close()


# --------------------------------------------------------------------------- what the walks found
def test_gpu_migrate_carries_the_sweep_floor():
    """The pair (SWEEP, MIGRATE) reduced: walk 3 failed at step 5, its first
    MIGRATE after a sweep, the target's scan reporting time_floor 0. rl_import leaves
    the target's floor alone, and limiter.migrate did not carry the source's
    over, so a request below it, which the source refuses (the sweep may have
    evicted that window's key), was counted from zero by the target."""
    T = W.NOW0
    kw = dict(max_batch=1 << 10, max_rules=8)
    a = Backend(0.8, False, table_slots=1 << 10, **kw)
    b = Backend(0.8, False, table_slots=1 << 11, hash_seed=3, n_shards=2, shard_devices=[0, 0], **kw)
    c = Backend(0.8, False, table_slots=1 << 10, **kw)
    try:
        old, keep = [b"floor_old_%03d_" % j for j in range(40)], [b"floor_keep_%03d_" % j for j in range(60)]
        insert(a, old, unit=1, now=T, hits=3)
        insert(a, keep, unit=2, now=T + 30)
        assert a.sweep(T + 10) == len(old)
        tot = migrate(a, b)
        assert tot["keys"] == len(keep) and tot["time_floor"] == T + 10
        assert sorted(SC.export_list(b)) == sorted(SC.export_list(a))  # (the target's sweep evicted nothing)
        n = len(old)
        below = arrays_from_lists(old, [T + 9] * n, list(range(n)), [1] * n, [0] * n, [1000] * n, [1] * n, [0] * n)
        for be in (a, b):
            assert {d["time_floor"] for _, d, _ in be.scan()} == {T + 10}
            assert (be.lookup(old, [1] * n, [T + 9] * n)["status"] == abi.RL_E_TIME).all()
            assert (be.do_limit_arrays(below, n, n, 1, isolate=True)["status"] == abi.RL_E_TIME).all()
            assert be.table_info()["live_slots"] == len(keep)
        # a target with a higher floor of its own keeps it
        c.sweep(T + 100)
        migrate(a, c)
        assert {d["time_floor"] for _, d, _ in c.scan()} == {T + 100}
    finally:
        for be in (a, b, c):
            be.close()


# --------------------------------------------------------------------------- scan cursors across the calls that keep them
def test_gpu_scan_cursor_survives_forget_sweep_relog_and_arena():
    """rl_resize and rl_snapshot_load invalidate a scan's cursor; every other
    call keeps it valid. A paged scan of a 2^13 table with rl_forget, rl_sweep
    (which compacts the arena), rl_resize_history and rl_resize_arena between
    its pages: every key that was there throughout comes exactly once, and no
    forgotten or evicted key comes on a page fetched after its removal."""
    T = W.NOW0
    be = Backend(0.8, False, table_slots=1 << 13, max_batch=1 << 12, max_rules=8, history_entries=1 << 16,
                 arena_bytes=1 << 18)
    try:
        def stems(tag, n):
            return [b"cur_%s_%05d_" % (tag, j) + (b"long_tail_" * 4 if j % 7 == 3 else b"") for j in range(n)]
        keep, forgotten, swept = stems(b"keep", 3000), stems(b"forget", 300), stems(b"sweep", 300)
        insert(be, keep + forgotten, unit=2, now=T)
        insert(be, swept, unit=1, now=T)               # SECOND keys: expired at T + 5
        insert(be, keep[::3], unit=2, now=T + 60)      # a third of the keys get a chain
        ops = [lambda: be.forget(forgotten)["keys"], lambda: be.sweep(T + 5),
               lambda: be.resize_history(4 << 16)["chains"], lambda: be.resize_arena(1 << 19)]
        want = [300, 300, 1000, None]
        pages, removed = [], set()
        for rec, d, _ in be.scan(page_records=700):    # (a tile holds about 450 keys: a page is one tile)
            part = SC.rec_list(rec)
            late = {r[0] for r in part} & removed
            assert not late, ("removed keys on a later page", len(pages), sorted(late)[:3])
            pages.append(part)
            if len(pages) <= len(ops):
                assert ops[len(pages) - 1]() == want[len(pages) - 1], len(pages)
                removed |= set((forgotten, swept)[len(pages) - 1]) if len(pages) <= 2 else set()
        assert len(pages) > len(ops) + 1
        groups = SC.groups_of([r for p in pages for r in p])  # (asserts: no key on two pages)
        seen = [g[0][0] for g in groups]
        assert sorted(s for s in seen if s.startswith(b"cur_keep_")) == sorted(keep)  # each once, none left out
        assert sum(len(g) == 2 for g in groups) == 1000 and all(len(g) <= 2 for g in groups)
        # some of the removed keys lay in tiles the scan had not reached: they are the ones it must not return
        assert len([s for s in seen if not s.startswith(b"cur_keep_")]) < 300
        assert be.table_info()["live_slots"] == 3000
    finally:
        be.close()
