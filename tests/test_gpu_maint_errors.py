"""The argument errors of the maintenance calls, pinned: return code and
rl_last_error text of every refusal the calls' host-side checks can give, in a
fixed order, on a ctx of one shard and on one of two.

The expected list (tests/golden/own_maint_errors.json) was recorded with this
module's case list against the library as it was before the calls' host side
was gathered into one layer:

    python tests/test_gpu_maint_errors.py --record

Every case also checks that the refused call changed nothing rl_table_info_get
shows and that a valid call of the same entry point succeeds right after it.
No case needs a device allocation to fail or a kernel to misbehave.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ratelimit_amd import abi
from ratelimit_amd.limiter import Backend

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "own_maint_errors.json")
T = 1_000_000          # the clock of the keys and of the sweep that sets the floor
SLOTS, BATCH, STEM_CAP, LOG, ARENA = 1024, 64, 4096, 4096, 1 << 16
DAY = 4
KEYS = [b"maint_err_key_%02d_" % i for i in range(8)] + [b"maint_err_long_" + b"x" * 200]


def _ctx(shards):
    be = Backend(0.8, False, table_slots=SLOTS, max_batch=BATCH, max_rules=8, max_stem_bytes=STEM_CAP,
                 history_entries=LOG, arena_bytes=ARENA, n_shards=shards, shard_devices=[0] * shards)
    be.restore(KEYS, [DAY] * len(KEYS), [T] * len(KEYS), [3] * len(KEYS))
    be.sweep(T)  # (the floor is now T: a read below it is refused)
    return be


def _csr(lens=None, off=None, size=None):
    """-> (bytes array, offsets array) of a stem list; off overrides the offsets."""
    if off is None:
        off = np.concatenate([[0], np.cumsum(lens)])
    off = np.ascontiguousarray(off, np.uint32)
    return np.full(max(int(size if size is not None else off.max()), 1), ord("k"), np.uint8), off


def _records(n, lens=None, off=None, null=(), stem_cap=None, unit=1, ws=0):
    blob, off = _csr(lens if lens is not None else [4] * n, off, stem_cap)
    a = {"stem_bytes": blob, "stem_off": off, "unit": np.full(max(n, 1), unit, np.uint8),
         "flags": np.zeros(max(n, 1), np.uint8), "ws": np.full(max(n, 1), ws, np.uint32),
         "count": np.ones(max(n, 1), np.uint32), "expire": np.full(max(n, 1), T + 86400, np.uint32),
         "lc": np.zeros(max(n, 1), np.uint32)}
    r = abi.RlRecords()
    r.n, r.stem_cap = n, blob.size if stem_cap is None else stem_cap
    for k, v in a.items():
        setattr(r, k, None if k in null else abi.ptr(v))
    return r, a


def _export(be, shard=0, out=None, info=True, **kw):
    r, keep = _records(**kw) if out else (None, None)
    inf = abi.RlExportInfo()
    return be.L.rl_export_range(be.ctx, shard, 0, SLOTS, C.byref(r) if out else None, C.byref(inf) if info else None)


def _import(be, none=False, ctx=True, **kw):
    r, keep = _records(**kw)
    return be.L.rl_import(be.ctx if ctx else None, None if none else C.byref(r))


def _lookup(be, n=2, lens=None, off=None, null=(), no_in=False, no_out=False):
    blob, off = _csr(lens if lens is not None else [4] * n, off)
    a = {"stem_bytes": blob, "stem_off": off, "unit": np.full(max(n, 1), DAY, np.uint8),
         "now": np.full(max(n, 1), T, np.int64)}
    k = abi.RlKeys()
    k.n = n
    for f, v in a.items():
        setattr(k, f, None if f in null else abi.ptr(v))
    res = {f: np.zeros(max(n, 1), dt) for f, dt in abi.KEY_STATE_DTYPES.items()}
    s = abi.RlKeyState()
    for f, v in res.items():
        setattr(s, f, None if f in null else abi.ptr(v))
    return be.L.rl_lookup(be.ctx, None if no_in else C.byref(k), None if no_out else C.byref(s))


def _hot(be, k=2, now=T, mask=0, flags=0, out=True, null=(), no_q=False, no_info=False, ctx=True):
    q = abi.RlHotQuery()
    q.now, q.k, q.unit_mask, q.flags = now, k, mask, flags
    r, keep = _records(min(k, BATCH), stem_cap=1 << 16, null=null)
    info = abi.RlHotInfo()
    return be.L.rl_hot_keys(be.ctx if ctx else None, None if no_q else C.byref(q), C.byref(r) if out else None,
                            None if no_info else C.byref(info))


def _forget(be, n=1, lens=None, off=None, flags=abi.RL_FORGET_DRY_RUN, null=(), none=False, ctx=True, key=None):
    blob, off = _csr(lens if lens is not None else [4] * n, off)
    if key is not None:
        blob, off = np.frombuffer(key, np.uint8).copy(), np.array([0, len(key)], np.uint32)
    s = abi.RlStems()
    s.n, s.flags = n, flags
    s.stem_bytes = None if "stem_bytes" in null else abi.ptr(blob)
    s.stem_off = None if "stem_off" in null else abi.ptr(off)
    removed = np.zeros(max(n, 1), np.uint32)
    info = abi.RlForgetInfo()
    return be.L.rl_forget(be.ctx if ctx else None, None if none else C.byref(s), abi.ptr(removed), C.byref(info))


def _scan(be, n=0, lens=None, off=None, flags=0, now=0, mask=0, reserved=0, null=(), no_q=False, no_cur=False,
          cur=(0, 0, 0), out=None, ctx=True):
    blob, off = _csr(lens if lens is not None else [4] * n, off)
    q = abi.RlScanQuery()
    q.n_prefixes, q.flags, q.now, q.unit_mask, q.reserved = n, flags, now, mask, reserved
    q.prefix_bytes = None if "prefix_bytes" in null else abi.ptr(blob)
    q.prefix_off = None if "prefix_off" in null else abi.ptr(off)
    c = abi.RlScanCursor()
    c.shard, c.reserved, c.slot = cur
    r, keep = _records(**out) if out else (None, None)
    byp = np.zeros((max(n, 1), 3), np.uint64)
    info = abi.RlScanInfo()
    return be.L.rl_scan(be.ctx if ctx else None, None if no_q else C.byref(q), None if no_cur else C.byref(c),
                        C.byref(r) if out else None, abi.ptr(byp), C.byref(info))


def _restore(be, off=None, none=False):
    blob, off = _csr(None, off if off is not None else [0, 4, 8, 12])
    n = len(off) - 1
    a = [np.full(n, DAY, np.uint8), np.full(n, T, np.int64), np.ones(n, np.uint32)]
    r = abi.RlRestoreBatch()
    r.n, r.stem_bytes, r.stem_off = n, abi.ptr(blob), abi.ptr(off)
    r.unit, r.now, r.count = (abi.ptr(x) for x in a)
    return be.L.rl_restore(be.ctx, None if none else C.byref(r))


def _resize(be, slots, ctx=True):
    return be.L.rl_resize(be.ctx if ctx else None, slots, C.byref(abi.RlResizeInfo()))


def _relog(be, entries, ctx=True):
    return be.L.rl_resize_history(be.ctx if ctx else None, entries, C.byref(abi.RlHistoryResizeInfo()))


def _arena(be, nbytes, ctx=True):
    return be.L.rl_resize_arena(be.ctx if ctx else None, nbytes)


BIG = 1 << 33  # a clock beyond the u32 range
PFX = abi.RL_FORGET_PREFIX | abi.RL_FORGET_DRY_RUN

# (entry point, its valid call, [(case, the refused call)]): issued in this order.
# The order is part of the fixture. On a ctx of one shard the refusals that
# rl_api.hip makes through plain `fail` (export_range.null_info and
# .shard_out_of_range, import.null_in, lookup.null_in and .null_out,
# restore.null_batch) leave rl_last_error at the engine's previous text, so the
# one-shard list expects the text of the case before them (DESIGN.md section 11,
# open item). Reordering or adding cases, or moving those calls to fail_call,
# changes these expectations and needs a new recording: that is no regression.
FAMILIES = [
    ("export_range", lambda be: _export(be), [
        ("null_info", lambda be: _export(be, info=False)),
        ("shard_out_of_range", lambda be: _export(be, shard=be.n_shards())),
        ("null_stem_off", lambda be: _export(be, out=True, n=4, null=("stem_off",))),
        ("null_column", lambda be: _export(be, out=True, n=4, null=("count",))),
        ("null_stem_bytes", lambda be: _export(be, out=True, n=4, null=("stem_bytes",))),
    ]),
    ("import", lambda be: _import(be, n=0), [
        ("null_ctx", lambda be: _import(be, ctx=False, n=1)),
        ("null_in", lambda be: _import(be, none=True, n=1)),
        ("count_over_cap", lambda be: _import(be, n=BATCH + 1, null=("unit",))),
        ("null_column", lambda be: _import(be, n=2, null=("expire",))),
        ("off0_not_0", lambda be: _import(be, n=2, off=[1, 4, 8])),
        ("empty_first", lambda be: _import(be, n=3, off=[0, 0, 4, 8])),
        ("decrease_middle", lambda be: _import(be, n=3, off=[0, 8, 4, 12])),
        ("empty_last", lambda be: _import(be, n=3, off=[0, 4, 8, 8])),
        ("entry_65536", lambda be: _import(be, n=2, lens=[4, 65536])),
        ("unit_0", lambda be: _import(be, n=2, unit=0)),
        ("unit_5", lambda be: _import(be, n=2, unit=5)),
        ("ws_off_window", lambda be: _import(be, n=2, unit=2, ws=61)),
        ("bytes_over_cap", lambda be: _import(be, n=2, lens=[2049, 2048])),
    ]),
    ("lookup", lambda be: _lookup(be), [
        ("null_in", lambda be: _lookup(be, no_in=True)),
        ("null_out", lambda be: _lookup(be, no_out=True)),
        ("count_over_cap", lambda be: _lookup(be, n=BATCH + 1, null=("unit",))),
        ("null_keys_array", lambda be: _lookup(be, null=("now",))),
        ("null_state_array", lambda be: _lookup(be, null=("found",))),
        ("off0_not_0", lambda be: _lookup(be, off=[2, 4, 8])),
        ("decrease_middle", lambda be: _lookup(be, n=3, off=[0, 8, 4, 12])),
        ("decrease_last", lambda be: _lookup(be, n=3, off=[0, 4, 8, 6])),
        ("bytes_over_cap", lambda be: _lookup(be, lens=[4000, 97])),
    ]),
    ("hot_keys", lambda be: _hot(be), [
        ("null_ctx", lambda be: _hot(be, ctx=False)),
        ("null_q", lambda be: _hot(be, no_q=True)),
        ("null_info", lambda be: _hot(be, no_info=True)),
        ("null_out", lambda be: _hot(be, out=False)),
        ("null_column", lambda be: _hot(be, null=("lc",))),
        ("null_stem_bytes", lambda be: _hot(be, null=("stem_bytes",))),
        ("unknown_flags", lambda be: _hot(be, flags=2)),
        ("unit_mask", lambda be: _hot(be, mask=1 << 5)),
        ("blocked_without_cache", lambda be: _hot(be, flags=abi.RL_HOT_BLOCKED)),
        ("k_over_cap", lambda be: _hot(be, k=BATCH + 1)),
        ("now_negative", lambda be: _hot(be, now=-1)),
        ("now_beyond", lambda be: _hot(be, now=BIG)),
        ("now_below_floor", lambda be: _hot(be, now=T - 1)),
    ]),
    ("resize", lambda be: _resize(be, SLOTS), [
        ("null_ctx", lambda be: _resize(be, SLOTS, ctx=False)),
        ("not_power_of_two", lambda be: _resize(be, 1000)),
        ("one_slot", lambda be: _resize(be, 1)),
        ("beyond_2_32", lambda be: _resize(be, 1 << 33)),
    ]),
    ("forget", lambda be: _forget(be, key=KEYS[0]), [
        ("null_ctx", lambda be: _forget(be, ctx=False)),
        ("null_in", lambda be: _forget(be, none=True)),
        ("unknown_flags", lambda be: _forget(be, flags=4)),
        ("count_over_cap", lambda be: _forget(be, n=BATCH + 1, null=("stem_off",))),
        ("prefixes_over_cap", lambda be: _forget(be, n=65, flags=PFX, null=("stem_off",))),
        ("null_stem_bytes", lambda be: _forget(be, null=("stem_bytes",))),
        ("null_stem_off", lambda be: _forget(be, flags=PFX, null=("stem_off",))),
        ("off0_not_0", lambda be: _forget(be, n=2, off=[3, 4, 8])),
        ("empty_first", lambda be: _forget(be, n=3, off=[0, 0, 4, 8])),
        ("decrease_middle", lambda be: _forget(be, n=3, off=[0, 8, 4, 12], flags=PFX)),
        ("empty_last", lambda be: _forget(be, n=3, off=[0, 4, 8, 8])),
        ("entry_65536", lambda be: _forget(be, n=1, lens=[65536])),
        ("bytes_over_cap", lambda be: _forget(be, n=2, lens=[4096, 1])),
        ("prefix_bytes_over_cap", lambda be: _forget(be, n=2, lens=[4096, 1], flags=PFX)),
    ]),
    ("scan", lambda be: _scan(be), [
        ("null_ctx", lambda be: _scan(be, ctx=False)),
        ("null_q", lambda be: _scan(be, no_q=True)),
        ("null_cursor", lambda be: _scan(be, no_cur=True)),
        ("cursor_reserved", lambda be: _scan(be, cur=(0, 1, 0))),
        ("cursor_shard_beyond", lambda be: _scan(be, cur=(be.n_shards() + 1, 0, 0))),
        ("unknown_flags", lambda be: _scan(be, flags=4)),
        ("reserved", lambda be: _scan(be, reserved=1)),
        ("unit_mask", lambda be: _scan(be, mask=1)),
        ("prefixes_over_cap", lambda be: _scan(be, n=65, null=("prefix_off",))),
        ("null_prefix_bytes", lambda be: _scan(be, n=1, null=("prefix_bytes",))),
        ("null_prefix_off", lambda be: _scan(be, n=1, null=("prefix_off",))),
        ("off0_not_0", lambda be: _scan(be, n=2, off=[1, 4, 8])),
        ("empty_first", lambda be: _scan(be, n=3, off=[0, 0, 4, 8])),
        ("decrease_middle", lambda be: _scan(be, n=3, off=[0, 8, 4, 12])),
        ("empty_last", lambda be: _scan(be, n=3, off=[0, 4, 8, 8])),
        ("bytes_over_cap", lambda be: _scan(be, n=2, lens=[4096, 1])),
        ("now_negative", lambda be: _scan(be, flags=abi.RL_SCAN_LIVE, now=-1)),
        ("now_beyond", lambda be: _scan(be, flags=abi.RL_SCAN_LIVE, now=BIG)),
        ("null_stem_off", lambda be: _scan(be, out=dict(n=4, null=("stem_off",)))),
        ("null_column", lambda be: _scan(be, out=dict(n=4, null=("ws",)))),
        ("null_stem_bytes", lambda be: _scan(be, out=dict(n=4, null=("stem_bytes",)))),
        ("finished_cursor_slot", lambda be: _scan(be, cur=(be.n_shards(), 0, abi.RL_SCAN_TILE))),
        ("cursor_off_grid", lambda be: _scan(be, cur=(0, 0, 5))),
        ("cursor_beyond_shard", lambda be: _scan(be, cur=(0, 0, 2 * SLOTS))),
        ("now_below_floor", lambda be: _scan(be, flags=abi.RL_SCAN_LIVE, now=T - 1)),
    ]),
    ("resize_history", lambda be: _relog(be, LOG), [
        ("null_ctx", lambda be: _relog(be, LOG, ctx=False)),
        ("zero", lambda be: _relog(be, 0)),
        ("beyond_2_31", lambda be: _relog(be, 1 << 40)),
    ]),
    ("resize_arena", lambda be: _arena(be, ARENA), [
        ("null_ctx", lambda be: _arena(be, ARENA, ctx=False)),
        ("zero", lambda be: _arena(be, 0)),
        ("not_multiple_of_16", lambda be: _arena(be, 24)),
        ("beyond_2_36", lambda be: _arena(be, 1 << 37)),
        ("bytes_in_use", lambda be: _arena(be, 16)),
    ]),
    ("restore", lambda be: _restore(be), [
        ("null_batch", lambda be: _restore(be, none=True)),
        # (a ctx of one shard leaves the offsets to the device's validation: routed ctx only)
        ("offsets_decrease_routed", lambda be: _restore(be, off=[0, 8, 4, 12]) if be.n_shards() > 1 else None),
    ]),
]


def run_cases(shards):
    """-> [[case id, return code, rl_last_error text]] of every refused call, in order."""
    be = _ctx(shards)
    got = []
    try:
        for name, valid, cases in FAMILIES:
            for case, call in cases:
                before = be.table_info()
                rc = call(be)
                if rc is None:
                    continue
                null_ctx = case == "null_ctx"
                msg = be.L.rl_last_error(None if null_ctx else be.ctx).decode()
                print("%d shard(s) %s.%s -> %d %r" % (shards, name, case, rc, msg))
                got.append(["%s.%s" % (name, case), rc, msg])
                assert rc != abi.RL_OK, "%s.%s was not refused" % (name, case)
                assert be.table_info() == before, "%s.%s changed the table" % (name, case)
                assert valid(be) == abi.RL_OK, "a valid %s after %s: %s" % (name, case, be.L.rl_last_error(be.ctx))
    finally:
        be.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [1, 2])
def test_maintenance_argument_errors_are_as_recorded(shards):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"][str(shards)]
    got = run_cases(shards)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_maint_errors.py --record")
    rec = {str(s): run_cases(s) for s in (1, 2)}
    with open(GOLDEN) as f:
        doc = json.load(f)  # (its kind and comment stay)
    doc["cases"] = rec
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("recorded %d + %d cases" % (len(rec["1"]), len(rec["2"])))
