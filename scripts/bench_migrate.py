"""Export / import rate (rl_export_range, rl_import): fills a C1-shaped table
(tenants x {SECOND, MINUTE} keys, BASELINE C1: 10M tenants in 2^27 slots)
through the workload generators, then times, with the host clock around calls
that end in a synchronise:

  * rl_table_info_get: the existing full-table scan (64 B per slot read), the
    yardstick of the export's scan kernels;
  * a full export into pinned host buffers, range by range;
  * a full import of those records into a fresh ctx of twice the slots.

    python scripts/bench_migrate.py [--tenants N] [--slots-log2 K] [--windows W]

Prints one JSON line. Under `rocprofv3 --kernel-trace --stats` the kernels
k_table_info, k_export_count, k_export_write and k_import give the device side.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ratelimit_amd import abi, workloads as W  # noqa: E402
from ratelimit_amd.limiter import Backend, PinnedArena  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=10_000_000)
    ap.add_argument("--slots-log2", type=int, default=27)
    ap.add_argument("--windows", type=int, default=2, help="passes over the tenants, one second apart (history)")
    ap.add_argument("--chunk-slots-log2", type=int, default=22)
    ap.add_argument("--batch", type=int, default=500_000, help="requests per fill batch")
    a = ap.parse_args()
    cap = 1 << 20
    src = Backend(0.8, False, table_slots=1 << a.slots_log2, max_batch=cap, max_rules=8, hash_seed=1)
    t0 = time.perf_counter()
    for w in range(a.windows):
        for lo in range(0, a.tenants, a.batch):
            src.do_limit_arrays(*W.c1_batch(np.arange(lo, min(lo + a.batch, a.tenants)), W.NOW0 + w))
    fill_s = time.perf_counter() - t0
    src.table_info()  # (warm)
    t0 = time.perf_counter()
    info = src.table_info()
    info_s = time.perf_counter() - t0

    # sizes first (rl_export_range without buffers), then pinned buffers for the largest range
    chunk = 1 << a.chunk_slots_log2
    ranges = [(lo, lo + chunk) for lo in range(0, 1 << a.slots_log2, chunk)]
    import ctypes as C
    need_n = need_b = 0
    t0 = time.perf_counter()
    for lo, hi in ranges:
        xi = abi.RlExportInfo()
        src._check(src.L.rl_export_range(src.ctx, 0, lo, hi, None, C.byref(xi)))
        need_n, need_b = max(need_n, xi.records), max(need_b, xi.stem_bytes)
    count_s = time.perf_counter() - t0
    pin = PinnedArena()
    bufs = {"stem_bytes": pin.array(need_b, np.uint8), "stem_off": pin.array(need_n + 1, np.uint32)}
    for k, dt in abi.RECORD_DTYPES.items():
        bufs[k] = pin.array(need_n, dt)
    parts, tot = [], {"records": 0, "stem_bytes": 0, "keys": 0, "chains_lost": 0}
    export_s = 0.0
    for lo, hi in ranges:
        t0 = time.perf_counter()
        rec, xi = src.export_range(0, lo, hi, bufs)
        export_s += time.perf_counter() - t0
        for k in tot:
            tot[k] += xi[k]
        parts.append({k: v.copy() for k, v in rec.items()})  # (kept for the import; not timed)
    src.close()
    copied = tot["stem_bytes"] + tot["records"] * (4 + 1 + 1 + 4 * 4)

    dst = Backend(0.8, False, table_slots=1 << (a.slots_log2 + 1), max_batch=cap, max_rules=8, hash_seed=2)
    t0 = time.perf_counter()
    calls = sum(dst.import_records(p) for p in parts)
    import_s = time.perf_counter() - t0
    after = dst.table_info()
    dst.close()
    pin.close()
    assert after["live_slots"] == info["live_slots"] == tot["keys"], (after, info, tot)
    print(json.dumps({
        "table_slots": 1 << a.slots_log2, "keys": tot["keys"], "records": tot["records"],
        "chains_lost": tot["chains_lost"], "fill_s": round(fill_s, 2),
        "table_info_ms": round(info_s * 1e3, 3), "table_info_GBps": round((64 << a.slots_log2) / info_s / 1e9, 1),
        "export_ranges": len(ranges), "export_sizing_s": round(count_s, 3), "export_s": round(export_s, 3),
        "export_records_per_s": round(tot["records"] / export_s), "export_bytes_copied": copied,
        "export_d2h_GBps": round(copied / export_s / 1e9, 2),
        "import_calls": calls, "import_s": round(import_s, 3), "import_records_per_s": round(tot["records"] / import_s),
        "dst_history_refused": after["history_refused"]}))


if __name__ == "__main__":
    main()
