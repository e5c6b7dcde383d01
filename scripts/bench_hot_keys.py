"""rl_hot_keys against the existing full-table scan: fills a C1-shaped table
(tenants x {SECOND, MINUTE} keys, BASELINE C1: 10M tenants in 2^27 slots) with
skewed counters (almost every key counted once, one tenant in a thousand up to
a few hundred times), then times, with the host clock around calls that end in
a synchronise:

  * rl_table_info_get: the existing scan of the same 64 B per slot, the yardstick;
  * rl_hot_keys for k in {10, 1000, 65536} x min_count in {0, 2};
  * one blocked run (RL_HOT_BLOCKED, k = 1000) on a second table filled with the
    local cache on, where the busy tenants' SECOND keys went over their limit.

    python scripts/bench_hot_keys.py [--tenants N] [--slots-log2 K] [--reps R]

Each figure is the median of R calls after a warm one. Prints one JSON line;
ratio = the call's time over the yardstick's. Under `rocprofv3 --kernel-trace
--stats` the kernels k_table_info, k_hot_scan, k_hot_select, k_hot_size and
k_hot_gather give the device side.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ratelimit_amd import workloads as W  # noqa: E402
from ratelimit_amd.limiter import Backend  # noqa: E402

KS = (10, 1000, 65536)
MIN_COUNTS = (0, 2)


def fill(be, tenants, batch, now):
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    for lo in range(0, tenants, batch):
        ten = np.arange(lo, min(lo + batch, tenants))
        hits = np.ones(ten.size, np.uint32)
        busy = ten % 1000 == 0
        hits[busy] = rng.integers(101, 400, int(busy.sum()))  # (over the SECOND limit of 100: blocked with the cache on)
        be.do_limit_arrays(*W.c1_batch(ten, now, hits))
    return time.perf_counter() - t0


def timed(f, reps):
    f()  # (warm)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, min(ts) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=10_000_000)
    ap.add_argument("--slots-log2", type=int, default=27)
    ap.add_argument("--batch", type=int, default=500_000, help="requests per fill batch")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    now = W.NOW0
    out = {"table_slots": 1 << a.slots_log2, "tenants": a.tenants, "reps": a.reps, "cases": []}
    for lc in (False, True):
        be = Backend(0.8, lc, table_slots=1 << a.slots_log2, max_batch=1 << 20, max_rules=8, hash_seed=1)
        fill_s = fill(be, a.tenants, a.batch, now)
        info_ms, info_min, info = timed(be.table_info, a.reps)
        if not lc:
            out.update(fill_s=round(fill_s, 2), keys=info["live_slots"], table_info_ms=round(info_ms, 3),
                       table_info_min_ms=round(info_min, 3),
                       table_info_GBps=round((64 << a.slots_log2) / (info_ms / 1e3) / 1e9, 1))
            runs = [(k, mc, False) for k in KS for mc in MIN_COUNTS]
        else:
            out.update(blocked_table_info_ms=round(info_ms, 3))
            runs = [(1000, 0, True)]
        for k, mc, blocked in runs:
            ms, ms_min, (rec, hi) = timed(lambda: be.hot_keys(now, k, mc, None, blocked), a.reps)
            n = len(rec["ws"])
            assert n == min(k, hi["matched"]) and (n == 0 or int(rec["count"][0]) >= int(rec["count"][-1]))
            out["cases"].append({"k": k, "min_count": mc, "blocked": blocked, "ms": round(ms, 3),
                                 "min_ms": round(ms_min, 3), "ratio": round(ms / info_ms, 2), "returned": n,
                                 "matched": hi["matched"], "threshold": hi["threshold"]})
        be.close()
    out["worst_ratio"] = max(c["ratio"] for c in out["cases"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
