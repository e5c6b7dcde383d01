"""rl_resize: the counter table grown, shrunk or rehashed in place on the GPU.

A Redis dictionary grows by itself; this table is sized at rl_create and answers
RL_E_TABLE_FULL when a key's probe window holds no slot. rl_resize places every
live slot in a table of another size on the device and re-points the history
log's entries at the keys' new slots; the ctx, its log, arena, gauges and
counters stay. What must hold:
  - a stream continues bit-exactly across the call (one C oracle replays all
    of it), whether the table grows, shrinks, keeps its size or is sharded;
  - the exported records, rl_lookup's answers and rl_table_info say the same
    before and after, but for table_slots and the tombstones, which are gone;
  - a table that is full takes new keys after growing;
  - a call that cannot place every key changes nothing at all.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle
from ratelimit_amd import abi, workloads as W
from ratelimit_amd.limiter import Backend, PinnedArena, RedisError
from ratelimit_amd.packing import PackedBatch, arrays_from_lists
from test_gpu_history import _stream
from test_gpu_migrate import STREAMS, _check, _export_all

pytestmark = pytest.mark.gpu

T = W.NOW0
FULL = abi.RL_E_TABLE_FULL
KW = dict(table_slots=1 << 18, max_batch=1 << 14, max_rules=8, hash_seed=11)
# name: (ctx arguments, the new per-shard slot count)
VARIANTS = {
    "grow": (KW, 1 << 20),
    "shrink": (KW, 1 << 16),
    "same": (KW, 1 << 18),
    "two_shards_grow": (dict(KW, n_shards=2, shard_devices=[0, 0]), 1 << 20),
}
UNCHANGED = ("live_slots", "exact_stems", "history_slots", "arena_bytes_used", "history_entries", "history_appended",
             "history_lost", "history_refused", "batches", "decisions")


def _stem(tag, j, length=20):
    s = b"%s_%07d_" % (tag, j)
    return (s + b"abcdefghijklmnopqrstuvwxyz0123456789" * (length // 36 + 1))[:length]


def _batch(stems, units, now, limit=1000, hits=1):
    n = len(stems)
    units = list(units) if isinstance(units, (list, tuple)) else [units] * n
    a = arrays_from_lists(list(stems), [now] * n, list(range(n)), units, [0] * n, [limit] * n, [hits] * n,
                          [u - 1 for u in units])
    return a, n, n, 2


def _do(be, co, bt, what):
    _check(be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt), what)


def _older_windows(recs, limit=300):
    """(stems, units, clocks) of up to `limit` records that are not their key's newest."""
    stems, units, nows = [], [], []
    for r, nxt in zip(recs, recs[1:]):
        if (r[0], r[1]) == (nxt[0], nxt[1]) and len(stems) < limit:
            stems.append(r[0])
            units.append(r[1])
            nows.append(r[3])
    return stems, units, nows


def _continue_across(which, variant, deep):
    mk, lc, jitter = STREAMS[which]
    batches = mk()
    kw, new_slots = VARIANTS[variant]
    shards = kw.get("n_shards", 1)
    be = Backend(0.8, lc, jitter=jitter, **kw)
    co = c_oracle.COracle(0.8, lc, horizon=jitter)
    try:
        half = len(batches) // 2
        for i, (x, n, nq, nr) in enumerate(batches[:half]):
            _check(be.do_limit_arrays(x, n, nq, nr, isolate=True), co.do_limit(x, n, nq, nr), i)
        ia = be.table_info()
        assert ia["history_appended"] > 0 and ia["exact_stems"] > 0
        if deep:
            ra, ta = _export_all(be)
            assert ta["records"] > ta["keys"]
            probe = _older_windows(ra)
            assert len(probe[0]) >= 20
            la = be.lookup(*probe)
            size_a = be.snapshot().size
        info = be.resize(new_slots)
        ib = be.table_info()
        assert info["slots_before"] == ia["table_slots"] == shards << 18
        assert info["slots_after"] == ib["table_slots"] == shards * new_slots
        assert info["keys"] == ia["live_slots"] and info["tombstones_dropped"] == ia["tombstones"]
        assert info["log_entries_relinked"] > 0 and ib["tombstones"] == 0
        assert info["longest_probe"] < min(new_slots, 1 << 16)
        for k in UNCHANGED:
            assert ia[k] == ib[k], k
        if deep:
            rb, tb = _export_all(be)
            assert sorted(ra) == sorted(rb) and ta == tb  # (windows, counts, expire, lc and the chain-lost flags)
            lb = be.lookup(*probe)
            for k in la:
                assert np.array_equal(la[k], lb[k]), k
            assert la["found"].any()
            assert be.snapshot().size - size_a == shards * (new_slots - (1 << 18)) * 64
        for i, (x, n, nq, nr) in enumerate(batches[half:]):
            _check(be.do_limit_arrays(x, n, nq, nr, isolate=True), co.do_limit(x, n, nq, nr), half + i)
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 1. continuation parity
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("which", ["alias_expire", "lc1", "lc1_j300"])
def test_gpu_resize_continues_bit_exactly(which, variant):
    """First half of the stream, rl_resize, second half on the same ctx: every
    batch equals ONE oracle replaying the whole stream. The streams move chains
    (clocks up to 7 windows back) and alias groups (stems under two units)."""
    _continue_across(which, variant, deep=False)


# --------------------------------------------------------------------------- 2. state equality
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gpu_resize_keeps_records_lookups_and_info(variant):
    """Around the same resize: the export's records, rl_lookup at the clocks of
    keys' older windows, every rl_table_info field but table_slots / tombstones,
    and rl_snapshot_size following the new count."""
    _continue_across("lc1_j300", variant, deep=True)


# --------------------------------------------------------------------------- 3. rescue of a full table
def test_gpu_resize_rescues_a_full_table():
    """2^10 slots (the probe window is the whole table) filled with 1024 keys: 64
    new keys are RL_E_TABLE_FULL, every one; after resize(2^11) they go in."""
    be = Backend(0.8, False, table_slots=1 << 10, max_batch=1 << 10, max_rules=8, hash_seed=77)
    co = c_oracle.COracle(0.8, False)
    try:
        first = [_stem(b"first", j) for j in range(1024)]
        for lo in range(0, 1024, 256):
            _do(be, co, _batch(first[lo:lo + 256], 1, T), "fill %d" % lo)
        assert be.table_info()["live_slots"] == 1024
        new = [_stem(b"new", j) for j in range(64)]
        g = be.do_limit_arrays(*_batch(new, 1, T), isolate=True)
        assert (g["status"] == FULL).all(), g["status"]
        info = be.resize(1 << 11)
        assert info["keys"] == 1024 and info["slots_after"] == 1 << 11 and info["tombstones_dropped"] == 0
        bt = _batch(new, 1, T)
        g = be.do_limit_arrays(*bt, isolate=True)
        _check(g, co.do_limit(*bt), "resubmitted")
        assert (g["limit_remaining"] == 999).all()  # count 1 each: the refused attempt counted nothing
        _do(be, co, _batch(first[::3] + new + [_stem(b"more", j) for j in range(100)], 1, T, hits=2), "old and new")
        assert be.table_info()["live_slots"] == 1024 + 64 + 100
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 4. tombstone purge
def test_gpu_resize_to_the_same_size_drops_the_tombstones():
    """2^12 slots, 2048 SECOND keys and 64 stems under SECOND and MINUTE; a sweep
    two seconds later leaves the SECOND keys nobody asked for again as
    tombstones (nearly half the table is empty, so the sweep reclaims none)."""
    be = Backend(0.8, True, table_slots=1 << 12, max_batch=1 << 11, max_rules=8, hash_seed=78, jitter=30)
    co = c_oracle.COracle(0.8, True, horizon=30)
    try:
        keys = [_stem(b"churn", j, 20 + 30 * (j % 3)) for j in range(2048)]  # (20, 50 and 80 bytes: slot and arena)
        alias = [_stem(b"alias", j) for j in range(64)]
        _do(be, co, _batch(keys[:1024], 1, T), "fill 0")
        _do(be, co, _batch(keys[1024:], 1, T), "fill 1")
        _do(be, co, _batch(alias + alias, [1] * 64 + [2] * 64, T, limit=5, hits=3), "alias")
        keep = keys[::10]
        _do(be, co, _batch(keep + alias, 1, T + 2, limit=5, hits=3), "keepers")
        assert be.sweep(T + 2) == 2048 - len(keep)
        ia = be.table_info()
        assert ia["tombstones"] == 2048 - len(keep) and ia["live_slots"] == len(keep) + 128 and ia["exact_stems"] == 128
        ra, ta = _export_all(be)
        info = be.resize(1 << 12)
        assert info["tombstones_dropped"] == ia["tombstones"] and info["keys"] == ia["live_slots"]
        ib = be.table_info()
        assert ib["tombstones"] == 0 and ib["table_slots"] == 1 << 12
        for k in UNCHANGED:
            assert ia[k] == ib[k], k
        rb, tb = _export_all(be)
        assert sorted(ra) == sorted(rb) and ta == tb
        _do(be, co, _batch(keep[::2] + alias + keys[1:400:10], 1, T + 2, limit=5, hits=1), "after")
        _do(be, co, _batch(alias + keep[:50], 2, T + 3, limit=5, hits=1), "minute")
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- 5. failure is atomic
def _info_raw(be, slots):
    info = abi.RlResizeInfo()
    return be.L.rl_resize(be.ctx, slots, C.byref(info)), info


def test_gpu_resize_failure_changes_nothing():
    be = Backend(0.8, True, table_slots=1 << 12, max_batch=1 << 11, max_rules=8, hash_seed=79, jitter=30)
    co = c_oracle.COracle(0.8, True, horizon=30)
    try:
        keys = [_stem(b"atomic", j) for j in range(1500)]
        _do(be, co, _batch(keys, 1, T, limit=5, hits=3), "T")
        _do(be, co, _batch(keys[::2], 1, T + 1, limit=5, hits=3), "T + 1")  # (chains: the log would be re-pointed)
        ia = be.table_info()
        assert ia["live_slots"] == 1500 and ia["history_appended"] > 0
        # (ranges of 1024 slots: one workgroup writes a range's records, in slot order)
        ra, ta = _export_all(be, chunk=1 << 10)
        snap = be.snapshot()
        with pytest.raises(RedisError, match="RL_E_TABLE_FULL") as ei:
            be.resize(1 << 10)
        assert ei.value.status == FULL
        rc, info = _info_raw(be, 1 << 10)  # (and once more through the raw call: the info is not written)
        assert rc == FULL and info.slots_after == 0 and info.keys == 0
        for bad in (3000, 0, 1, (1 << 12) + 1):
            rc, _ = _info_raw(be, bad)
            assert rc == abi.RL_E_INVALID, bad
        rb, tb = _export_all(be, chunk=1 << 10)
        assert ra == rb and ta == tb  # the same order: the slot array is the old one
        assert be.table_info() == ia
        assert np.array_equal(be.snapshot(), snap)
        _do(be, co, _batch(keys[::3] + [_stem(b"fresh", j) for j in range(200)], 1, T + 1, limit=5, hits=1), "next")
        assert be.L.rl_resize(be.ctx, 1 << 13, None) == abi.RL_OK  # (info may be NULL)
        assert be.table_info()["table_slots"] == 1 << 13
        _do(be, co, _batch(keys[::4], 1, T, limit=5, hits=1), "after the grow, a second back")
    finally:
        be.close()
        co.close()


def test_gpu_resize_no_shard_commits_unless_all_placed():
    """Two shards of 2^12 slots filled until one holds more than 1024 keys and the
    other does not: resize(2^10) fits one shard only, so neither may change."""
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=1 << 11, max_rules=8, hash_seed=80, n_shards=2,
                 shard_devices=[0, 0])
    co = c_oracle.COracle(0.8, False)
    try:
        keys = [_stem(b"shard", j) for j in range(2400)]
        _do(be, co, _batch(keys[:1900], 1, T), "fill")
        n, live = 1900, [be.table_info(j)["live_slots"] for j in (0, 1)]
        while max(live) <= 1024:
            _do(be, co, _batch(keys[n:n + 8], 1, T), "fill %d" % n)
            n, live = n + 8, [be.table_info(j)["live_slots"] for j in (0, 1)]
        assert min(live) <= 1024 < max(live) and sum(live) == n, live
        ia = [be.table_info(j) for j in (0, 1)]
        ra, ta = _export_all(be, chunk=1 << 10)
        rc, info = _info_raw(be, 1 << 10)
        assert rc == FULL and info.slots_after == 0
        assert [be.table_info(j) for j in (0, 1)] == ia and ia[0]["table_slots"] == ia[1]["table_slots"] == 1 << 12
        rb, tb = _export_all(be, chunk=1 << 10)
        assert ra == rb and ta == tb
        _do(be, co, _batch(keys[:n:3], 1, T, hits=2), "next")
        info = be.resize(1 << 11)
        assert info["keys"] == n and info["slots_before"] == 2 << 12 and info["slots_after"] == 2 << 11
        assert [be.table_info(j)["table_slots"] for j in (0, 1)] == [1 << 11] * 2
        _do(be, co, _batch(keys[1:n:3] + keys[n:], 1, T, hits=2), "after")
    finally:
        be.close()
        co.close()


def test_gpu_resize_not_on_a_communicator_ctx():
    from ratelimit_amd.sharded import loopback_id
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=64, max_rules=8)
    try:
        uid = loopback_id()
        be._check(be.L.rl_comm_init(be.ctx, 1, 0, abi.ptr(uid)))
        rc, info = _info_raw(be, 1 << 13)
        assert rc == abi.RL_E_INVALID and info.slots_after == 0
        assert be.table_info()["table_slots"] == 1 << 12
    finally:
        be.close()


# --------------------------------------------------------------------------- 6. snapshot across sizes
def test_gpu_resize_then_snapshot_loads_at_the_new_size():
    kw = dict(max_batch=1 << 12, max_rules=8, jitter=300, hash_seed=3, history_entries=1 << 16)
    a = Backend(0.8, True, table_slots=1 << 16, **kw)
    b = Backend(0.8, True, table_slots=1 << 17, **kw)
    small = Backend(0.8, True, table_slots=1 << 16, **kw)
    try:
        for x, n, nq, nr in _stream(5, 500, 1_000, 6, 20, 150, multi=True):
            a.do_limit_arrays(x, n, nq, nr, isolate=True)  # (only the state it leaves matters here)
        assert a.table_info()["history_appended"] > 0
        a.resize(1 << 17)
        ra, ta = _export_all(a)
        assert ta["records"] > ta["keys"] > 0
        snap = a.snapshot()
        b.load_snapshot(snap)
        rb, tb = _export_all(b)
        assert sorted(ra) == sorted(rb) and ta == tb
        assert small.L.rl_snapshot_load(small.ctx, abi.ptr(snap), snap.size) == abi.RL_E_INVALID
    finally:
        a.close()
        b.close()
        small.close()


# --------------------------------------------------------------------------- 7. ordering
def test_gpu_resize_orders_after_batches_in_flight():
    """Four host-fed batches submitted without waiting, rl_resize at once (it
    must order after them and hold the pipeline), three more batches, one
    synchronize: all seven are the oracle's."""
    batches = _stream(31, 1_500, 2_500, 7, 3, 7, multi=True, hot=200)
    co = c_oracle.COracle(0.8, True)
    want = [co.do_limit(*b) for b in batches]
    co.close()
    be = Backend(0.8, True, table_slots=1 << 14, max_batch=1 << 13, max_rules=8, hash_seed=13)
    arena = PinnedArena()
    try:
        keep = []
        for i, (a, n, nq, nr) in enumerate(batches):
            if i == 4:
                info = be.resize(1 << 16)
                assert info["keys"] > 0 and info["log_entries_relinked"] > 0
            pb = PackedBatch({k: arena.like(v) for k, v in a.items()}, n, nq, nr)
            out = {k: arena.like(v) for k, v in pb.alloc_result(True).items()}
            keep.append((pb, out, be.do_limit_host_async(pb, out)))
        be.synchronize()
        for i, ((pb, out, _), w) in enumerate(zip(keep, want)):
            g = {k: out[k][:pb.n] for k in ("code", "limit_remaining", "reset_s", "status")}
            g["stats"] = out["stats"][:pb.n_rules * abi.RL_NUM_STATS]
            _check(g, w, i)
        assert be.table_info()["table_slots"] == 1 << 16
    finally:
        be.close()
        arena.close()
