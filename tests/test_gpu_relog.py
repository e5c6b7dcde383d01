"""rl_resize_history and rl_resize_arena: the history log rebuilt at another
size from the live chains, and the long-stem arena re-allocated, on the GPU.

The log is sized at rl_create; when it is too small, lookups that reach an
overwritten entry are RL_E_TIME and rl_table_info.history_lost / _refused
count. rl_resize_history copies what a lookup's walk accepts of every live
key's chain into a log of another size and drops everything else. What must
hold:
  - a stream continues bit-exactly across the call (one C oracle replays all
    of it), whether the log grows, shrinks, keeps its size or is sharded;
  - the exported records (the chain-lost flags included), rl_lookup's answers,
    rl_table_info but for history_entries, and the gauges say the same before
    and after;
  - entries no live chain reaches are gone and counted; a chain the log had cut
    stays cut in the same place, and never miscounts;
  - a ctx whose log is too small for its stream stops losing once grown;
  - a call that does not fit changes nothing at all.
rl_resize_arena is the same remedy for RL_E_ARENA_FULL.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle
from ratelimit_amd import abi, workloads as W
from ratelimit_amd.limiter import Backend, PinnedArena, RedisError
from ratelimit_amd.packing import PackedBatch, arrays_from_lists
import streams
from test_gpu_alias import _stream as _alias_stream
from test_gpu_history import _stream
from test_gpu_migrate import STREAMS, _check, _export_all

pytestmark = pytest.mark.gpu

T = W.NOW0
SMALLEST = 1 << 16  # 64 partitions x 1024 entries
KW = dict(table_slots=1 << 18, max_batch=1 << 14, max_rules=8, hash_seed=11)
# The smallest log on which a stream is exact by itself. The J = 300 stream's
# exact path (stems under two units, a hot key replayed serially) sends a few
# partitions more appends in a batch than the smallest log's 1024 a partition
# admits: log_append refuses them (history_refused) with or without any call
# of this file, as tests/test_gpu_migrate.py notes for its own variants; 4096 a
# partition is what tests/test_gpu_resize.py runs the stream on.
FLOOR = {"alias_expire": SMALLEST, "lc1": SMALLEST, "lc1_j300": 4 * SMALLEST}
# name: (ctx arguments, the log at creation and the new history_entries per shard, in floors)
VARIANTS = {
    "grow_4x": (KW, 1, 4),
    "same": (KW, 1, 1),
    "shrink_to_smallest": (KW, 4, 1),
    "two_shards_grow": (dict(KW, n_shards=2, shard_devices=[0, 0]), 1, 4),
}
DIV = {1: 1, 2: 60, 3: 3600, 4: 86400}


def _raw(be, entries):
    info = abi.RlHistoryResizeInfo()
    return be.L.rl_resize_history(be.ctx, entries, C.byref(info)), info


def _desc_batch(stems, units, nows, limit=1000, hits=1):
    """One request per descriptor, each at its own clock."""
    n = len(stems)
    units = list(units) if isinstance(units, (list, tuple, np.ndarray)) else [units] * n
    nows = list(nows) if isinstance(nows, (list, tuple, np.ndarray)) else [nows] * n
    a = arrays_from_lists(list(stems), [int(t) for t in nows], list(range(n)), [int(u) for u in units], [0] * n,
                          [limit] * n, [hits] * n, [int(u) - 1 for u in units])
    return a, n, n, 4


def _long_stem(tag, j, length=80):
    s = b"%s_%07d_" % (tag, j)
    return (s + b"abcdefghijklmnopqrstuvwxyz0123456789" * 3)[:length]


def _older_windows(recs, limit=300):
    """(stems, units, clocks) of up to `limit` records that are not their key's newest."""
    stems, units, nows = [], [], []
    for r, nxt in zip(recs, recs[1:]):
        if (r[0], r[1]) == (nxt[0], nxt[1]) and len(stems) < limit:
            stems.append(r[0])
            units.append(r[1])
            nows.append(r[3])
    return stems, units, nows


def _same_export(a, b):
    """Two exports (_export_all's pairs) hold the same records and sums. The order between
    workgroups' records is the export's own, so the lists are compared sorted;
    a difference is reported by its first record, not by a diff of 10^5 tuples."""
    (ra, ta), (rb, tb) = a, b
    assert ta == tb, (ta, tb)
    sa, sb = sorted(ra), sorted(rb)
    if sa != sb:
        k = next(i for i, (x, y) in enumerate(zip(sa, sb)) if x != y)
        raise AssertionError("exports differ at sorted record %d: %r != %r" % (k, sa[k], sb[k]))


def _second_keys(tenants, now):
    a, n, nq, nr = W.c1_batch(tenants, now)
    a["unit"][:] = 1  # both stems of a tenant under SECOND: two single-unit keys per tenant
    return a, n, nq, nr


def _exact_or_time(be, co, bt):
    """The batch on be; the oracle is fed the descriptors that succeeded alone.
    Every other one is RL_E_TIME. -> the failed mask."""
    a, n, nq, nr = bt
    g = be.do_limit_arrays(a, n, nq, nr, isolate=True)
    failed = g["status"] != 0
    assert (g["status"][failed] == abi.RL_E_TIME).all(), np.unique(g["status"])
    o = co.do_limit(*streams.drop_descriptors(a, n, nq, ~failed), nr)
    for k in ("code", "limit_remaining", "reset_s"):
        assert np.array_equal(g[k][~failed], o[k]), k
    return failed


def _continue_across(which, variant, deep):
    mk, lc, jitter = STREAMS[which]
    batches = mk()
    kw, at_create, after = VARIANTS[variant]
    kw, new_entries = dict(kw, history_entries=at_create * FLOOR[which]), after * FLOOR[which]
    shards = kw.get("n_shards", 1)
    be = Backend(0.8, lc, jitter=jitter, **kw)
    co = c_oracle.COracle(0.8, lc, horizon=jitter)
    try:
        half = len(batches) // 2
        for i, (x, n, nq, nr) in enumerate(batches[:half]):
            _check(be.do_limit_arrays(x, n, nq, nr, isolate=True), co.do_limit(x, n, nq, nr), i)
        ia = be.table_info()
        assert ia["history_appended"] > 0 and ia["history_entries"] == shards * kw["history_entries"]
        if deep:
            now = int(batches[half - 1][0]["now"].max())
            ra, ta = _export_all(be)
            assert ta["records"] > ta["keys"]
            probe = _older_windows(ra)
            assert len(probe[0]) >= 20
            la = be.lookup(*probe)
            ga = be.local_cache_info(now)
        info = be.resize_history(new_entries)
        ib = be.table_info()
        print(which, variant, info)
        assert info["entries_before"] == ia["history_entries"]
        assert info["entries_after"] == ib["history_entries"] == shards * new_entries
        assert info["chains"] == ia["history_slots"] and info["entries_kept"] >= info["chains"] - info["chains_lost"]
        assert info["entries_kept"] + info["entries_dropped"] == info["written_before"] <= ia["history_appended"]
        assert info["fill_max"] <= new_entries // 64 and info["longest_chain"] >= 1
        for k in ia:  # history_appended, _lost, _refused, history_slots, arena_bytes_used and the rest
            assert ia[k] == ib[k] or k == "history_entries", k
        if deep:
            rb, tb = _export_all(be)
            _same_export((ra, ta), (rb, tb))  # (windows, counts, expire, lc and the chain-lost flags)
            assert info["chains_lost"] == ta["chains_lost"]
            assert info["entries_kept"] >= ta["records"] - ta["keys"]  # (every version of a window is kept)
            lb = be.lookup(*probe)
            for k in la:
                assert np.array_equal(la[k], lb[k]), k
            assert la["found"].any()
            assert be.local_cache_info(now) == ga
        for i, (x, n, nq, nr) in enumerate(batches[half:]):
            _check(be.do_limit_arrays(x, n, nq, nr, isolate=True), co.do_limit(x, n, nq, nr), half + i)
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 1. continuation parity
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("which", ["alias_expire", "lc1", "lc1_j300"])
def test_gpu_relog_continues_bit_exactly(which, variant):
    """First half of the stream, rl_resize_history, second half on the same ctx:
    every batch equals ONE oracle replaying the whole stream. The streams move
    chains (clocks up to 7 windows back; 299 s under J = 300) and alias groups
    (stems under two units, whose windows have several versions on a chain)."""
    _continue_across(which, variant, deep=False)


# --------------------------------------------------------------------------- 2. state equality
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gpu_relog_keeps_records_lookups_info_and_gauges(variant):
    _continue_across("lc1_j300", variant, deep=True)


# --------------------------------------------------------------------------- 3. garbage goes, counted right
def test_gpu_relog_drops_and_counts_the_garbage():
    """The smallest log under generations of SECOND keys: each generation's 3000
    keys are hit in four consecutive seconds (three appends a key, every entry
    an older window's only version: no clock runs back), then swept, which
    leaves their 9000 entries in the log with no chain to reach them. Ten
    generations append 90 000 entries to a log of 65 536: partitions wrap, onto
    garbage and onto the oldest generations' entries alike. The last two
    generations are not swept: their chains are what an equal-size call keeps."""
    be = Backend(0.8, False, table_slots=1 << 16, max_batch=1 << 13, max_rules=8, hash_seed=5, history_entries=1)
    try:
        assert be.table_info()["history_entries"] == SMALLEST
        gens = 10
        for g in range(gens):
            ten = np.arange(1500) + 10_000 * g
            for s in range(4):
                out = be.do_limit_arrays(*_second_keys(ten, T + 10 * g + s), isolate=True)
                assert (out["status"] == 0).all()
            if g < gens - 2:
                assert be.sweep(T + 10 * g + 6) == 3000
        ia = be.table_info()
        assert ia["live_slots"] == 6000 and ia["history_appended"] == gens * 9000 and ia["history_lost"] == 0
        ra, ta = _export_all(be)
        info = be.resize_history(SMALLEST)
        print(info)
        assert info["written_before"] < ia["history_appended"]  # (some partition had wrapped)
        assert info["entries_kept"] == ta["records"] - ta["keys"] == 2 * 9000 and ta["chains_lost"] == 0
        assert info["entries_dropped"] > 0 and info["chains"] == 6000 and info["chains_lost"] == 0
        assert info["entries_kept"] + info["entries_dropped"] == info["written_before"]
        assert info["fill_max"] <= info["entries_after"] // 64 and info["longest_chain"] == 3
        ib = be.table_info()
        assert ib == ia
        rb, tb = _export_all(be)
        _same_export((ra, ta), (rb, tb))
        again = be.resize_history(SMALLEST)  # nothing left to drop
        assert again["entries_dropped"] == 0 and again["written_before"] == again["entries_kept"] == info["entries_kept"]
    finally:
        be.close()


# --------------------------------------------------------------------------- 4. lost chains stay lost
@pytest.mark.parametrize("lc", [False, True])
def test_gpu_relog_lost_chains_stay_lost_never_miscount(lc):
    """The far-too-small log of test_gpu_alias (64 x 1024 entries, J = 300, alias
    groups), wrapped: chains are cut, some at their very head (a key whose only
    record left is its newest window, flagged). After a 16x grow the export is
    the same, flags included; lookups that were RL_E_TIME are RL_E_TIME, and so
    are requests into those windows; everything else is the oracle's."""
    be = Backend(0.8, lc, table_slots=1 << 17, max_batch=1 << 14, max_rules=8, history_entries=1, jitter=300)
    co = c_oracle.COracle(0.8, lc, horizon=300)
    try:
        assert be.table_info()["history_entries"] == SMALLEST
        batches = _alias_stream(list(range(38, 98)) + list(range(40, 70)), rpb=8_000, tenants=30_000, seed=21)
        for bt in batches[:60]:
            _exact_or_time(be, co, bt)
        r0, t0 = _export_all(be)
        assert t0["chains_lost"] > 0
        per_key = {}
        for r in r0:
            per_key.setdefault((r[0], r[1]), []).append(r)
        cut = [v[0] for v in per_key.values() if v[0][2]][:300]
        probe = ([r[0] for r in cut], [r[1] for r in cut], [r[3] - 1 for r in cut])  # the window below the oldest kept
        # requests into those windows before the call: the ones that fail count nothing and change nothing
        bt = _desc_batch(*probe)
        was_time = _exact_or_time(be, co, bt)
        assert was_time.any()
        ia = be.table_info()
        assert ia["history_appended"] > ia["history_entries"]  # the log wrapped
        ra, ta = _export_all(be)
        assert ta["chains_lost"] > 0
        per_key = {}
        for r in ra:
            per_key.setdefault((r[0], r[1]), []).append(r)
        assert any(len(v) == 1 and v[0][2] for v in per_key.values())  # cut at the head: nothing of the chain is left
        la = be.lookup(*probe)
        info = be.resize_history(16 * SMALLEST)
        print(info)
        rb, tb = _export_all(be)
        _same_export((ra, ta), (rb, tb))
        assert info["chains_lost"] == ta["chains_lost"] and info["chains"] == ia["history_slots"]
        ib = be.table_info()
        for k in ia:
            assert ia[k] == ib[k] or k == "history_entries", k
        lb = be.lookup(*probe)
        for k in la:
            assert np.array_equal(la[k], lb[k]), k
        idx = np.nonzero(was_time)[0]
        g = be.do_limit_arrays(*_desc_batch([probe[0][i] for i in idx], [probe[1][i] for i in idx],
                                            [probe[2][i] for i in idx]), isolate=True)
        assert (g["status"] == abi.RL_E_TIME).all(), np.unique(g["status"])
        failed = ok = 0
        for bt in batches[60:]:
            f = _exact_or_time(be, co, bt)
            failed, ok = failed + int(f.sum()), ok + int((~f).sum())
        assert ok > failed
        ic = be.table_info()
        assert ic["history_refused"] == ib["history_refused"]  # (a log of 2^20 refuses nothing of these batches)
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 5. the remedy works
def _remedy_stream():
    """2000 SECOND keys hit once a second for 24 s (J = 300: every window a key has
    had stays askable), so every batch appends 2000 entries, a wave's 64 to one
    partition: the 32 partitions in use take 64 a batch and the smallest log's
    1024 a partition are full after 16 batches. The first half (12 batches, 704
    a partition) fits. In the second half, from second 20 on, a quarter of the
    keys is also asked 20 s back: the walk to that window's entry, appended 19
    batches earlier, ends on one the log has overwritten. -> (first, second)"""
    ten = np.arange(1000)
    first = [_second_keys(ten, T + k) for k in range(12)]
    second = []
    for k in range(12, 24):
        second.append(_second_keys(ten, T + k))
        if k >= 20:
            second.append(_second_keys(ten[::4], T + k - 20))
    return first, second


def test_gpu_relog_growing_ends_the_losses():
    """One stream on two ctxs with the smallest log, one of them grown 16x half
    way. The untouched one loses history in the second half (RL_E_TIME answers,
    history_lost or history_refused rising: a property of the log's size); the
    grown one answers everything as the oracle does and its counters stay."""
    kw = dict(table_slots=1 << 16, max_batch=1 << 14, max_rules=8, history_entries=1, jitter=300, hash_seed=9)
    small, grown = Backend(0.8, True, **kw), Backend(0.8, True, **kw)
    co = c_oracle.COracle(0.8, True, horizon=300)
    try:
        first, second = _remedy_stream()
        half = len(first)
        for i, bt in enumerate(first):
            o = co.do_limit(*bt)
            _check(small.do_limit_arrays(*bt, isolate=True), o, i)
            _check(grown.do_limit_arrays(*bt, isolate=True), o, i)
        i_small, i_grown = small.table_info(), grown.table_info()
        assert i_small == i_grown and i_small["history_entries"] == SMALLEST
        info = grown.resize_history(16 * SMALLEST)
        print(info)
        assert info["chains_lost"] == 0 and grown.table_info()["history_entries"] == 16 * SMALLEST
        lost = 0
        for i, bt in enumerate(second):
            _check(grown.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt), half + i)
            g = small.do_limit_arrays(*bt, isolate=True)
            assert np.isin(g["status"], (0, abi.RL_E_TIME)).all()
            lost += int((g["status"] == abi.RL_E_TIME).sum())
        j_small, j_grown = small.table_info(), grown.table_info()
        print(lost, j_small, j_grown)
        assert lost > 0
        assert (j_small["history_lost"] + j_small["history_refused"] >
                i_small["history_lost"] + i_small["history_refused"])
        assert j_grown["history_lost"] == i_grown["history_lost"] == 0
        assert j_grown["history_refused"] == i_grown["history_refused"] == 0
    finally:
        small.close()
        grown.close()
        co.close()


# --------------------------------------------------------------------------- 6. a shrink that does not fit
@pytest.mark.parametrize("shards", [1, 2])
def test_gpu_relog_shrink_that_does_not_fit_changes_nothing(shards):
    """8000 tenants x 2 SECOND keys hit in six consecutive seconds: 80 000 live
    chain entries per ctx (per shard: all of them on one, half on two, so the
    two-shard ctx takes twice the tenants in two batches a second). The smallest
    log holds 65 536: some partition is asked for more than its 1024."""
    kw = dict(KW, history_entries=4 * SMALLEST, jitter=30)
    if shards > 1:
        kw.update(n_shards=shards, shard_devices=[0] * shards)
    be = Backend(0.8, True, **kw)
    co = c_oracle.COracle(0.8, True, horizon=30)
    try:
        groups = [np.arange(8000) + 8000 * s for s in range(shards)]
        for s in range(6):
            for ten in groups:
                bt = _second_keys(ten, T + s)
                _check(be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt), s)
        ia = be.table_info()
        assert ia["history_appended"] == shards * 80_000 and ia["history_slots"] == shards * 16_000
        snap = be.snapshot()
        with pytest.raises(RedisError, match="RL_E_CAPACITY") as ei:
            be.resize_history(SMALLEST)
        assert ei.value.status == abi.RL_E_CAPACITY
        rc, info = _raw(be, SMALLEST)  # (and once more through the raw call: the info is not written)
        assert rc == abi.RL_E_CAPACITY and info.entries_after == 0 and info.chains == 0
        assert be.table_info() == ia and int(be.cfg.history_entries) == 4 * SMALLEST
        assert np.array_equal(be.snapshot(), snap)
        for k, ten in enumerate(groups):  # on: forward, then back into logged windows
            for t in (T + 6, T + 3):
                bt = _second_keys(ten[::2], t)
                _check(be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt), "after %d %d" % (k, t))
        assert be.resize_history(2 * SMALLEST)["entries_after"] == shards * 2 * SMALLEST  # 2048 a partition: it fits
        bt = _second_keys(groups[0][1::2], T + 2)
        _check(be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt), "after the shrink that fits")
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 7. snapshot across sizes
def test_gpu_relog_then_snapshot_loads_at_the_new_size():
    kw = dict(table_slots=1 << 16, max_batch=1 << 12, max_rules=8, jitter=300, hash_seed=3)
    a = Backend(0.8, True, history_entries=SMALLEST, **kw)
    b = Backend(0.8, True, history_entries=4 * SMALLEST, **kw)
    try:
        for x, n, nq, nr in _stream(5, 500, 1_000, 6, 20, 150, multi=True):
            a.do_limit_arrays(x, n, nq, nr, isolate=True)  # (only the state it leaves matters here)
        assert a.table_info()["history_appended"] > 0
        before = a.snapshot()
        info = a.resize_history(4 * SMALLEST)
        ra, ta = _export_all(a)
        assert ta["records"] > ta["keys"] > 0
        snap = a.snapshot()
        # the slots, the counters, the kept entries: the log's unreachable entries are not in it
        assert before.size - snap.size == 32 * info["entries_dropped"]
        b.load_snapshot(snap)
        rb, tb = _export_all(b)
        _same_export((ra, ta), (rb, tb))
        assert b.table_info()["history_appended"] == info["entries_kept"]
        assert a.L.rl_snapshot_load(a.ctx, abi.ptr(before), before.size) == abi.RL_E_INVALID  # (the old geometry)
        assert b.L.rl_snapshot_load(b.ctx, abi.ptr(before), before.size) == abi.RL_E_INVALID
        a.load_snapshot(snap)
        _same_export(_export_all(a), (ra, ta))
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------- 8. ordering
def test_gpu_relog_orders_after_host_batches_in_flight():
    """Four host-fed batches submitted without waiting, rl_resize_history at once
    (it must order after them and hold the pipeline), three more batches, one
    synchronize: all seven are the oracle's."""
    batches = _stream(31, 1_500, 2_500, 7, 3, 7, multi=True, hot=200)
    co = c_oracle.COracle(0.8, True)
    want = [co.do_limit(*b) for b in batches]
    co.close()
    be = Backend(0.8, True, table_slots=1 << 14, max_batch=1 << 13, max_rules=8, hash_seed=13,
                 history_entries=SMALLEST)
    arena = PinnedArena()
    try:
        keep = []
        for i, (a, n, nq, nr) in enumerate(batches):
            if i == 4:
                info = be.resize_history(4 * SMALLEST)
                assert info["chains"] > 0 and info["entries_kept"] > 0
            pb = PackedBatch({k: arena.like(v) for k, v in a.items()}, n, nq, nr)
            out = {k: arena.like(v) for k, v in pb.alloc_result(True).items()}
            keep.append((pb, out, be.do_limit_host_async(pb, out)))
        be.synchronize()
        for i, ((pb, out, _), w) in enumerate(zip(keep, want)):
            g = {k: out[k][:pb.n] for k in ("code", "limit_remaining", "reset_s", "status")}
            g["stats"] = out["stats"][:pb.n_rules * abi.RL_NUM_STATS]
            _check(g, w, i)
        assert be.table_info()["history_entries"] == 4 * SMALLEST
    finally:
        be.close()
        arena.close()


def test_gpu_relog_orders_after_wire_batches_in_flight():
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
        first = be.resize_history(SMALLEST)  # (no synchronize before it: the second halves are pending)
        be.synchronize()
        for _, w, _, _ in keep:  # (a message with a limit override is deferred to the host path: not counted here)
            assert np.isin(w["req_status"], (abi.RL_WIRE_OK, abi.RL_WIRE_DEFERRED)).all()
        info = be.table_info()
        second = be.resize_history(SMALLEST)
        # nothing arrived after the first call (it had waited for all three), and it left no garbage
        assert first["chains"] == second["chains"] == info["history_slots"]
        assert first["entries_kept"] == second["entries_kept"] == second["written_before"]
        assert first["written_before"] == info["history_appended"] and info["live_slots"] > 100
    finally:
        arena.close()
        svc.close()


# --------------------------------------------------------------------------- 9. the arena
@pytest.mark.parametrize("shards", [1, 2])
def test_gpu_resize_arena_rescues_a_full_arena(shards):
    """4096 B of arena a shard hold the 48-B tails of 85 stems of 80 bytes: of 160
    such stems a shard (MINUTE keys) the rest are RL_E_ARENA_FULL, every one.
    After resize_arena to 4x they go in. Then rounds of 100 fresh SECOND long
    stems a shard with a sweep between rounds: 480 + 300 of a shard's 1024 units
    are live in a round, so the arena lasts only if each sweep compacts, and a
    sweep compacts the keepers' 480 units into the spare arena, which held 256."""
    kw = dict(table_slots=1 << 14, max_batch=1 << 12, max_rules=8, hash_seed=21, arena_bytes=4096)
    if shards > 1:
        kw.update(n_shards=shards, shard_devices=[0] * shards)
    be = Backend(0.8, False, **kw)
    co = c_oracle.COracle(0.8, False)
    try:
        stems = [_long_stem(b"keeper", j) for j in range(160 * shards)]
        a, n, nq, nr = _desc_batch(stems, 2, T)
        g = be.do_limit_arrays(a, n, nq, nr, isolate=True)
        full = g["status"] == abi.RL_E_ARENA_FULL
        assert full.sum() >= 160 * shards - 85 * shards and (g["status"][~full] == 0).all() and (~full).sum() >= 85
        o = co.do_limit(*streams.drop_descriptors(a, n, nq, ~full), nr)
        for k in ("code", "limit_remaining", "reset_s"):
            assert np.array_equal(g[k][~full], o[k]), k
        ia = be.table_info()
        assert ia["arena_bytes_used"] == 48 * int((~full).sum())
        ra, ta = _export_all(be)
        snap = be.snapshot()
        with pytest.raises(RedisError, match="RL_E_ARENA_FULL") as ei:
            be.resize_arena(2048)  # (below the bytes in use of some shard)
        assert ei.value.status == abi.RL_E_ARENA_FULL and int(be.cfg.arena_bytes) == 4096
        assert np.array_equal(be.snapshot(), snap) and be.table_info() == ia
        be.resize_arena(4 * 4096)
        assert be.table_info() == ia
        _same_export(_export_all(be), (ra, ta))
        refused = [s for s, f in zip(stems, full) if f]
        bt = _desc_batch(refused, 2, T)
        g = be.do_limit_arrays(*bt, isolate=True)
        _check(g, co.do_limit(*bt), "resubmitted")
        assert (g["limit_remaining"] == 999).all()  # count 1 each: the refused attempt counted nothing
        assert be.table_info()["arena_bytes_used"] == 48 * len(stems)
        for r in range(1, 5):
            fresh = [_long_stem(b"round%d" % r, j) for j in range(100 * shards)]
            bt = _desc_batch(stems + fresh, [2] * len(stems) + [1] * len(fresh), T + 10 * r)
            _check(be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt), "round %d" % r)
            assert be.sweep(T + 10 * r + 5) == len(fresh)
            assert be.table_info()["arena_bytes_used"] == 48 * len(stems)  # compacted: the keepers' tails alone
        bt = _desc_batch(stems[::3], 2, T + 50, hits=3)
        _check(be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt), "keepers after the rounds")
        snap = be.snapshot()  # the new size travels: a fresh ctx of that arena loads it
        kw["arena_bytes"] = 4 * 4096
        b2 = Backend(0.8, False, **kw)
        try:
            b2.load_snapshot(snap)
            _same_export(_export_all(b2), _export_all(be))
        finally:
            b2.close()
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 10. whole-call errors
def test_gpu_relog_and_arena_whole_call_errors():
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=64, max_rules=8, history_entries=SMALLEST,
                 arena_bytes=1 << 16)
    try:
        L = be.L
        assert L.rl_resize_history(None, SMALLEST, None) == abi.RL_E_INVALID
        assert L.rl_resize_arena(None, 1 << 16) == abi.RL_E_INVALID
        ia = be.table_info()
        for bad in (0, (1 << 31) + 1, 1 << 40):
            rc, info = _raw(be, bad)
            assert rc == abi.RL_E_INVALID and info.entries_after == 0, bad
        for bad in (0, 24, (1 << 16) + 8, (1 << 36) + 16):
            assert L.rl_resize_arena(be.ctx, bad) == abi.RL_E_INVALID, bad
        assert be.table_info() == ia
        # rounded as rl_create rounds: 1 is the smallest log, one entry a partition more doubles it
        assert L.rl_resize_history(be.ctx, 1, None) == abi.RL_OK  # (info may be NULL)
        assert be.table_info()["history_entries"] == SMALLEST
        assert be.resize_history(SMALLEST + 64)["entries_after"] == 2 * SMALLEST
        assert be.resize_history(1)["entries_before"] == 2 * SMALLEST
        assert L.rl_resize_arena(be.ctx, 16) == abi.RL_OK and L.rl_resize_arena(be.ctx, 1 << 16) == abi.RL_OK
    finally:
        be.close()


def test_gpu_relog_and_arena_not_on_a_communicator_ctx():
    from ratelimit_amd.sharded import loopback_id
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=64, max_rules=8, history_entries=SMALLEST)
    try:
        uid = loopback_id()
        be._check(be.L.rl_comm_init(be.ctx, 1, 0, abi.ptr(uid)))
        rc, info = _raw(be, 4 * SMALLEST)
        assert rc == abi.RL_E_INVALID and info.entries_after == 0
        assert be.L.rl_resize_arena(be.ctx, 1 << 20) == abi.RL_E_INVALID
        assert be.table_info()["history_entries"] == SMALLEST
    finally:
        be.close()
