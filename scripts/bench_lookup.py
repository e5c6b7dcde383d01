"""Keyed lookup rate (rl_lookup): fills a C1-shaped table (tenants x {SECOND,
MINUTE} keys, BASELINE C1: 10M tenants in 2^27 slots) through the workload
generators, then times, with the host clock around the synchronous call:

  * a lookup of --keys keys the table holds (the tenants' MINUTE keys, read in
    their window: found, with their counts), in random tenant order;
  * a lookup of --keys stems it never saw (probes that end at an empty slot).

    python scripts/bench_lookup.py [--tenants N] [--slots-log2 K] [--keys N] [--reps R]

Prints one JSON line: keys/s end to end of the C call on prebuilt arrays (the
best of --reps calls) and the time of one Backend.lookup on a list of stems. Under
`rocprofv3 --kernel-trace --stats` the kernel k_lookup gives the device side;
k_table of the fill batches (500k requests = 1M keys each) is the comparison.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ratelimit_amd import abi, workloads as W  # noqa: E402
from ratelimit_amd.limiter import Backend  # noqa: E402


def _timed(be, rows, units, nows, reps):
    """The C call alone on prebuilt arrays (best of reps), then Backend.lookup on
    a list of stems once (the Python mirror's packing included)."""
    n, L = rows.shape
    blob = np.ascontiguousarray(rows).reshape(-1)
    off = (np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32)
    res = {f: np.zeros(n, dt) for f, dt in abi.KEY_STATE_DTYPES.items()}
    k, s = abi.RlKeys(), abi.RlKeyState()
    k.n = n
    k.stem_bytes, k.stem_off, k.unit, k.now = abi.ptr(blob), abi.ptr(off), abi.ptr(units), abi.ptr(nows)
    for f, v in res.items():
        setattr(s, f, abi.ptr(v))
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        be._check(be.L.rl_lookup(be.ctx, C.byref(k), C.byref(s)))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    stems = [r.tobytes() for r in rows]
    t0 = time.perf_counter()
    res2 = be.lookup(stems, units, nows)
    py_s = time.perf_counter() - t0
    for f in res:
        assert np.array_equal(res[f], res2[f]), f
    return best, py_s, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=10_000_000)
    ap.add_argument("--slots-log2", type=int, default=27)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=500_000, help="requests per fill batch")
    a = ap.parse_args()
    cap = 1 << 20
    n = min(a.keys, cap)
    be = Backend(0.8, False, table_slots=1 << a.slots_log2, max_batch=cap, max_rules=8, hash_seed=1)
    t0 = time.perf_counter()
    for lo in range(0, a.tenants, a.batch):
        be.do_limit_arrays(*W.c1_batch(np.arange(lo, min(lo + a.batch, a.tenants)), W.NOW0))
    fill_s = time.perf_counter() - t0

    rng = np.random.default_rng(7)
    ten = rng.integers(0, a.tenants, n)
    x = W.c1_batch(ten, W.NOW0)[0]
    L = int(x["stem_off"][1])
    rows = x["stem_bytes"].reshape(2 * n, L)
    present = rows[1::2]  # the MINUTE stems
    absent = W.c1_batch(ten + a.tenants, W.NOW0)[0]["stem_bytes"].reshape(2 * n, L)[1::2]
    units, nows = np.full(n, 2, np.uint8), np.full(n, W.NOW0 + 5, np.int64)
    hit_s, hit_py_s, hit = _timed(be, present, units, nows, a.reps)
    miss_s, miss_py_s, miss = _timed(be, absent, units, nows, a.reps)
    info = be.table_info()
    be.close()
    assert not hit["status"].any() and hit["found"].all() and (hit["count"] >= 1).all()
    assert not miss["status"].any() and not miss["found"].any()
    print(json.dumps({
        "table_slots": 1 << a.slots_log2, "live_slots": info["live_slots"], "keys": n, "stem_bytes": L,
        "fill_s": round(fill_s, 2),
        "present_s": round(hit_s, 5), "present_keys_per_s": round(n / hit_s),
        "absent_s": round(miss_s, 5), "absent_keys_per_s": round(n / miss_s),
        "present_python_s": round(hit_py_s, 4), "absent_python_s": round(miss_py_s, 4)}))


if __name__ == "__main__":
    main()
