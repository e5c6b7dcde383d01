"""The counter table under key churn: sweeps make tombstones, new keys arrive,
round after round, in tables small enough to run out of empty slots.

What must hold (tests/table_model.py is the CPU model of the same rules):
  - an insert fails with RL_E_TABLE_FULL only when its probe window holds
    neither an empty slot nor a tombstone: a window that ends without an empty
    slot claims a tombstone, and a claim lost to another lane goes on to the
    next one;
  - rl_sweep, on a table short of empty slots, turns the tombstones no live key
    needs back into empty slots, and leaves every tombstone that lies between
    a live key's home and its slot;
  - answers stay those of the C oracle throughout.
Every batch is sent with isolate=True, so a key that finds no slot shows as its
descriptor's status.
"""
import numpy as np
import pytest

from oracle import c_oracle
from ratelimit_amd import abi, workloads as W
from ratelimit_amd.limiter import Backend
from ratelimit_amd.packing import arrays_from_lists
import table_model
from test_gpu_migrate import _export_all, _record_list

pytestmark = pytest.mark.gpu

T = W.NOW0
SLOTS = 1 << 10
KW = dict(table_slots=SLOTS, max_batch=1 << 10, max_rules=8, hash_seed=77)
FULL = abi.RL_E_TABLE_FULL
ANSWER = ("code", "limit_remaining", "reset_s")


def _stem(tag, j, length=20):
    """Distinct per (tag, j); tag at most 8 bytes."""
    s = b"%s_%07d_" % (tag, j)
    assert len(s) <= length
    return (s + b"abcdefghijklmnopqrstuvwxyz0123456789" * (length // 36 + 1))[:length]


def _batch(stems, units, now, limits, hits, rules=None, n_rules=1):
    n = len(stems)

    def col(v):
        return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n

    a = arrays_from_lists(list(stems), [now] * n, list(range(n)), col(units), [0] * n, col(limits), col(hits),
                          col(rules if rules is not None else 0))
    return a, n, n, n_rules


def _same(g, o, what):
    """Every status 0 and every answer the oracle's."""
    st, cnt = np.unique(g["status"], return_counts=True)
    assert not g["status"].any(), "%s: statuses %s x %s" % (what, [abi.STATUS_NAMES.get(int(x), x) for x in st], cnt)
    for k in ANSWER + ("stats",):
        bad = np.nonzero(g[k] != o[k])[0]
        assert bad.size == 0, "%s: %s differs at %s: gpu %s oracle %s" % (what, k, bad[:5], g[k][bad[:5]], o[k][bad[:5]])


def _do(be, co, bt, what):
    """The batch on the GPU and on the oracle."""
    g = be.do_limit_arrays(*bt, isolate=True)
    _same(g, co.do_limit(*bt), what)
    return g


def _empties(info):
    return info["table_slots"] - info["live_slots"] - info["tombstones"]


def _slot_stem(be, slot, shard=0):
    """The stem and unit of the key in one slot (a single-slot export)."""
    rec, _ = be.export_range(shard, slot, slot + 1)
    keys = {(r[0], r[1]) for r in _record_list(rec)}
    assert len(keys) == 1, (slot, keys)
    return keys.pop()


def _pairs(recs):
    """The export's (stem, unit) keys, each once (_export_all checked that a key's records are contiguous)."""
    out = []
    for r in recs:
        if not out or out[-1] != (r[0], r[1]):
            out.append((r[0], r[1]))
    assert len(set(out)) == len(out)
    return out


# --------------------------------------------------------------------------- A
def test_gpu_churn_a_table_of_nothing_but_tombstones_takes_keys():
    """1024 keys fill the 1024 slots, a sweep leaves 1024 tombstones and no live
    key: none of them is needed, so 512 new keys find a table of empty slots.
    (Before reclamation and the window-end claim: 512 x RL_E_TABLE_FULL.)"""
    be, co = Backend(0.8, False, **KW), c_oracle.COracle(0.8, False)
    try:
        first = [_stem(b"first", j) for j in range(1024)]
        for lo in range(0, 1024, 256):
            _do(be, co, _batch(first[lo:lo + 256], 1, T, 1000, 1), "fill %d" % lo)
        info = be.table_info()
        assert info["live_slots"] == 1024 and info["tombstones"] == 0
        assert be.sweep(T + 2) == 1024
        other = [_stem(b"other", j) for j in range(512)]
        _do(be, co, _batch(other, 1, T + 2, 1000, 2), "after the sweep")
        info = be.table_info()
        assert info["live_slots"] == 512 and info["tombstones"] == 0, info
        assert set(_pairs(_export_all(be)[0])) == {(s, 1) for s in other}
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- B
@pytest.mark.parametrize("length", [20, 60])
def test_gpu_churn_b_inserts_claim_needed_tombstones_and_only_a_full_table_is_full(length):
    """debug_hash_bits=2: the homes are slots 0, 256, 512 and 768. All 1024 slots
    are filled; the keys in slots 255, 511, 767 and 1023 survive the sweep. A
    key's path from its home covers at least its own quarter up to its slot, so
    each of the 1020 tombstones lies before a live key on that key's path: the
    sweep may free none, and there is no empty slot. 1020 new keys must still go
    in (each at the end of a window without an empty slot), then the table is
    full: three more keys fail, alone. Stems of 60 bytes keep their tails in the
    arena."""
    be = Backend(0.8, False, debug_hash_bits=2, arena_bytes=1 << 16, **KW)
    co = c_oracle.COracle(0.8, False)
    try:
        fill = [_stem(b"fill", j, length) for j in range(1024)]
        for lo in range(0, 1024, 256):
            _do(be, co, _batch(fill[lo:lo + 256], 1, T, 1000, 1), "fill %d" % lo)
        info = be.table_info()
        assert info["live_slots"] == 1024 and info["tombstones"] == 0
        keepers = [_slot_stem(be, s) for s in (255, 511, 767, 1023)]
        assert all(u == 1 for _, u in keepers) and len(set(keepers)) == 4
        keepers = [s for s, _ in keepers]
        _do(be, co, _batch(keepers, 1, T + 2, 1000, 3), "keepers")
        assert be.sweep(T + 2) == 1020
        info = be.table_info()
        assert info["tombstones"] == 1020 and info["live_slots"] == 4, info  # (every tombstone is needed)
        res = be.lookup(keepers, [1] * 4, [T + 2] * 4)
        assert not res["status"].any() and res["found"].all(), res
        assert list(res["count"]) == [3] * 4 and list(res["expire"]) == [T + 3] * 4

        new = [_stem(b"new", j, length) for j in range(1020)]
        for lo in range(0, 1020, 255):
            _do(be, co, _batch(new[lo:lo + 255], 1, T + 2, 1000, 2), "refill %d" % lo)
        info = be.table_info()
        assert info["live_slots"] == 1024 and info["tombstones"] == 0, info

        # full now: 3 further keys fail alone (their own rule: the oracle counts them, the table cannot)
        extra, present = [_stem(b"extra", j, length) for j in range(3)], new[100:150]
        stems = present[:25] + extra[:2] + present[25:] + extra[2:]
        is_extra = np.array([s in extra for s in stems])
        bt = _batch(stems, 1, T + 2, 1000, 1, rules=is_extra.astype(int), n_rules=2)
        g, o = be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt)
        assert (g["status"][is_extra] == FULL).all() and not g["status"][~is_extra].any(), g["status"]
        for k in ANSWER:
            assert np.array_equal(g[k][~is_extra], o[k][~is_extra]), k
        assert np.array_equal(g["stats"][:abi.RL_NUM_STATS], o["stats"][:abi.RL_NUM_STATS])
        # present keys in a table without an empty slot, whole-batch mode: absent units are no error
        bt = _batch(present, 1, T + 2, 1000, 1)
        g, o = be.do_limit_arrays(*bt), co.do_limit(*bt)
        for k in ANSWER + ("stats",):
            assert np.array_equal(g[k], o[k]), k

        recs, tot = _export_all(be)
        assert sorted(_pairs(recs)) == sorted((s, 1) for s in keepers + new) and tot["keys"] == 1024
        newest = {}
        for r in recs:
            newest[r[0]] = r  # (a key's records are oldest first)
        for s in keepers:
            assert newest[s][3:5] == (T + 2, 3), newest[s]
        info = be.table_info()
        assert info["live_slots"] == 1024 and info["tombstones"] == 0
    finally:
        be.close()
        co.close()


# --------------------------------------------------------------------------- C
N_ALIAS, N_CHURN, N_LONG, ROUNDS = 32, 448, 16, 40
LIM_SECOND, LIM_MINUTE = 5, 60


def _round_batch(rng, churn, alias, now):
    """Every live key 1 to 3 times with hits 1 to 4, shuffled: rule 0 = SECOND
    (limit 5), rule 1 = MINUTE (limit 60), both low enough for OVER_LIMIT."""
    keys = [(s, 1) for s in churn] + [(s, u) for s in alias for u in (1, 2)]
    rows = [k for k in keys for _ in range(int(rng.integers(1, 4)))]
    order = rng.permutation(len(rows))
    stems = [rows[j][0] for j in order]
    units = [rows[j][1] for j in order]
    return _batch(stems, units, now, [LIM_SECOND if u == 1 else LIM_MINUTE for u in units],
                  rng.integers(1, 5, len(rows)).tolist(), rules=[u - 1 for u in units], n_rules=2), keys


@pytest.mark.parametrize("lc", [False, True])
def test_gpu_churn_c_forty_rounds_against_the_oracle(lc):
    """512 live keys in 1024 slots: 448 SECOND stems, half of them replaced by
    stems never seen before in every round (16 of the 448 are 60 to 300 bytes
    long: the arena churns too), and 32 stems under SECOND and MINUTE that are
    hit in every round (the alias path). Round r is one batch at T + 3r, then
    rl_sweep at that clock: the keys not hit in the round die. One ctx with one
    shard, one with two shards of 1024 slots each; both must answer as the
    oracle does, sweep exactly the dropped keys, and keep empty slots.

    The bound on the empty slots after a sweep, from round 10 on:
    table_model.min_empties_after_sweep() is 153 of 1024 slots (32 seeds of the
    same churn on the CPU model); the GPU's inserts are concurrent and its
    homes come from another hash, so half of it, 76, is asked here, scaled to a
    shard's table. A table that never reclaims has 0 by then."""
    bound = table_model.gpu_empties_bound()
    rng = np.random.default_rng(5 + lc)
    kw = dict(KW, max_batch=1 << 11)  # (512 keys up to 3 times each)
    one = Backend(0.8, lc, jitter=0, **kw)
    two = Backend(0.8, lc, jitter=0, n_shards=2, shard_devices=[0, 0], **kw)
    co = c_oracle.COracle(0.8, lc)
    snap = None
    serial = [0]

    def fresh(long):
        serial[0] += 1
        return _stem(b"churn", serial[0], int(rng.integers(60, 301)) if long else 24)

    try:
        alias = [_stem(b"alias", j, 28) for j in range(N_ALIAS)]
        churn = [fresh(p < N_LONG) for p in range(N_CHURN)]  # (position p < N_LONG: a long stem)
        retired, low = [], {"one": SLOTS, "two": SLOTS}
        for r in range(ROUNDS):
            now = T + 3 * r
            dropped = []
            if r:
                for p in rng.choice(N_CHURN, N_CHURN // 2, replace=False):
                    dropped.append(churn[p])
                    churn[p] = fresh(p < N_LONG)
            bt, keys = _round_batch(rng, churn, alias, now)
            o = co.do_limit(*bt)
            for name, be in (("one", one), ("two", two)) + ((("snap", snap),) if snap else ()):
                _same(be.do_limit_arrays(*bt, isolate=True), o, "round %d (%s)" % (r, name))
            if snap:  # the snapshot of round 20 answered round 21 like the table it came from
                snap.close()
                snap = None
            for name, be in (("one", one), ("two", two)):
                assert be.sweep(now) == len(dropped), (r, name)
                info = be.table_info()
                assert info["live_slots"] == len(keys) == 512, (r, name, info)
                shards = [be.table_info(k) for k in range(be.n_shards())] if name == "two" else [info]
                for si in shards:
                    e = _empties(si) * SLOTS // si["table_slots"]
                    if r >= 10:
                        low[name] = min(low[name], e)
                        assert e >= bound, (r, name, si, bound)
            retired += dropped
            if r == 20:
                gone = retired[-200:]
                stems = [s for s, _ in keys] + gone
                units = [u for _, u in keys] + [1] * len(gone)
                for be in (one, two):
                    res = be.lookup(stems, units, [now] * len(stems))
                    assert not res["status"].any()
                    assert res["found"][:len(keys)].all() and not res["found"][len(keys):].any(), r
                snap = Backend(0.8, lc, jitter=0, **kw)
                snap.load_snapshot(one.snapshot())
        print("churn lc=%d: fewest empty slots per 1024 after a sweep, rounds 10..39: %s (bound %d)" % (lc, low, bound))

        # rl_import into the churned tables: 200 new keys, 50 present ones (their window overwritten)
        now = T + 3 * (ROUNDS - 1)  # (the last sweep's clock: the table holds the last round's keys, all live)
        imp = [_stem(b"import", j, 24 if j % 8 else 90) for j in range(200)] + churn[100:150]
        n = len(imp)
        count = (7 + np.arange(n)).astype(np.uint32)
        rec = {"stem_bytes": np.frombuffer(b"".join(imp), np.uint8).copy(),
               "stem_off": np.cumsum([0] + [len(s) for s in imp]).astype(np.uint32),
               "unit": np.ones(n, np.uint8), "flags": np.zeros(n, np.uint8), "ws": np.full(n, now, np.uint32),
               "count": count, "expire": np.full(n, now + 1, np.uint32), "lc": np.zeros(n, np.uint32)}
        want = sorted(set(keys) | {(s, 1) for s in imp})
        for be in (one, two):
            be.import_records(rec)
            res = be.lookup(imp, [1] * n, [now] * n)
            assert not res["status"].any() and res["found"].all()
            assert np.array_equal(res["count"], count) and (res["expire"] == now + 1).all()
            assert be.table_info()["live_slots"] == len(want) == 512 + 200
            assert sorted(_pairs(_export_all(be)[0])) == want  # the bookkeeping: the last round's keys and the imports
    finally:
        for be in (one, two, snap):
            if be:
                be.close()
        co.close()


# --------------------------------------------------------------------------- D
def test_gpu_churn_d_many_lanes_one_tombstone():
    """900 keys in 1024 slots die, except one MINUTE key per 64-slot stretch
    (found by export) whose paths keep tombstones in the table. 800 new keys in
    ONE batch then race for those tombstones and the empty slots: every one gets
    a slot of its own (a second batch reads the counts back: a key written over
    by another would start again). Then a batch of more new keys than there are
    free slots: exactly as many succeed as slots were free, the rest are
    RL_E_TABLE_FULL and nothing else."""
    be, co = Backend(0.8, False, **KW), c_oracle.COracle(0.8, False)
    try:
        first = [_stem(b"first", j) for j in range(900)]
        _do(be, co, _batch(first, 1, T, 1000, 1), "fill")
        # one stem per stretch: under MINUTE it takes the first empty slot after its cluster, the cluster on its path
        keep = []
        for lo in range(0, SLOTS, 64):
            rec, _ = be.export_range(0, lo, lo + 64)
            stems = [r[0] for r in _record_list(rec)]
            assert stems, lo
            keep.append(stems[-1])
        assert len(set(keep)) == 16
        _do(be, co, _batch(keep, 2, T, 1000, 5, rules=1, n_rules=2), "keepers")
        assert be.sweep(T + 2) == 900
        info = be.table_info()
        assert info["live_slots"] == 16 and info["tombstones"] >= 16, info  # (tombstones on the keepers' paths stay)
        res = be.lookup(keep, [2] * 16, [T + 2] * 16)
        assert not res["status"].any() and res["found"].all() and list(res["count"]) == [5] * 16

        new = [_stem(b"new", j) for j in range(800)]
        _do(be, co, _batch(new, 1, T + 2, 1000, 2), "800 at once")
        info = be.table_info()
        assert info["live_slots"] == 816, info
        assert sorted(_pairs(_export_all(be)[0])) == sorted([(s, 1) for s in new] + [(s, 2) for s in keep])
        _do(be, co, _batch(new + keep, [1] * 800 + [2] * 16, T + 2, 1000, 1, rules=[0] * 800 + [1] * 16, n_rules=2),
            "the counts read back")

        free = SLOTS - 816
        more = [_stem(b"more", j) for j in range(KW["max_batch"])]
        assert len(more) > free
        bt = _batch(more, 1, T + 2, 1000, 3)
        g, o = be.do_limit_arrays(*bt, isolate=True), co.do_limit(*bt)
        ok = g["status"] == 0
        assert int(ok.sum()) == free and (g["status"][~ok] == FULL).all(), np.unique(g["status"], return_counts=True)
        for k in ANSWER:
            assert np.array_equal(g[k][ok], o[k][ok]), k
        info = be.table_info()
        assert info["live_slots"] == SLOTS and info["tombstones"] == 0, info
        got = _pairs(_export_all(be)[0])
        assert sorted(got) == sorted([(s, 1) for s in new] + [(s, 2) for s in keep] +
                                     [(s, 1) for s, f in zip(more, ok) if f])
    finally:
        be.close()
        co.close()
