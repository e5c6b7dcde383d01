"""rl_scan against what the table offered for the same questions before it: fills
a C1-shaped table (tenants x {SECOND, MINUTE} keys, BASELINE C1: 10M tenants in
2^27 slots = 20M keys) as scripts/bench_forget.py does, then times, with the host
clock around synchronous calls on the same table in one process:

  * "which keys does this prefix hold": Backend.scan over all pages with a
    prefix that selects about one key in a thousand (tenants 0..9999), its
    count-only form Backend.count_keys, and the same answer the old way:
    Backend.export_records() of the whole table and a numpy prefix filter on
    the host;
  * "list everything": Backend.scan without a prefix in pages of 2^20 records,
    against Backend.export_records() alone;
  * the scans it is compared with on the device: rl_table_info_get and
    rl_forget's dry run with the same prefix.

    python scripts/bench_scan.py [--tenants N] [--slots-log2 K] [--reps R] [--export-reps E]

Prints one JSON line. Figures are the median of R calls after a warm one (the
export paths: of E). Under `rocprofv3 --kernel-trace --stats` the kernels
k_scan_count, k_scan_write, k_export_count, k_export_write, k_forget_scan and
k_table_info give the device side.
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


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=10_000_000)
    ap.add_argument("--slots-log2", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--export-reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=500_000, help="requests per fill batch")
    ap.add_argument("--page-records", type=int, default=1 << 20)
    return ap.parse_args(argv)


def selective_prefix(tenants):
    """-> (prefix, tenants whose two keys it selects): one key in a thousand of the default table."""
    if tenants > 10_000:
        return b"bench_tenant_t000000", 10_000
    return b"bench_tenant_t", tenants


def timed(f, reps):
    f()  # (warm)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, min(ts) * 1e3, r


def scan_pages(be, **kw):
    """Every page of Backend.scan -> (records, stem bytes, pages)."""
    n = nb = pages = 0
    for rec, info, _ in be.scan(**kw):
        n += len(rec["ws"])
        nb += len(rec["stem_bytes"])
        pages += 1
    return n, nb, pages


def export_all(be, prefix=None):
    """Backend.export_records() of the whole table (prefix: and the numpy filter
    for it on the host) -> (records kept, stem bytes moved)."""
    kept = moved = 0
    p = None if prefix is None else np.frombuffer(prefix, np.uint8)
    for part in be.export_records():
        off, blob = part["stem_off"], part["stem_bytes"]
        moved += len(blob)
        n = len(part["ws"])
        if p is None or not n:
            kept += n
            continue
        start = off[:-1].astype(np.int64)
        ok = (off[1:].astype(np.int64) - start) >= len(p)
        idx = np.flatnonzero(ok)
        if len(idx):  # the first len(p) bytes of every stem long enough, compared at once
            head = blob[(start[idx][:, None] + np.arange(len(p))[None, :]).reshape(-1)].reshape(-1, len(p))
            kept += int((head == p).all(axis=1).sum())
    return kept, moved


def main():
    a = parse_args()
    slots = 1 << a.slots_log2
    be = Backend(0.8, False, table_slots=slots, max_batch=1 << 20, max_rules=8, hash_seed=1)
    t0 = time.perf_counter()
    for lo in range(0, a.tenants, a.batch):
        be.do_limit_arrays(*W.c1_batch(np.arange(lo, min(lo + a.batch, a.tenants)), W.NOW0))
    out = {"table_slots": slots, "tenants": a.tenants, "reps": a.reps, "export_reps": a.export_reps,
           "fill_s": round(time.perf_counter() - t0, 2)}
    info_ms, _, info = timed(be.table_info, a.reps)
    out.update(keys=info["live_slots"], table_info_ms=round(info_ms, 3))
    prefix, sel = selective_prefix(a.tenants)
    dry_ms, _, dry = timed(lambda: be.forget([prefix], prefix=True, dry_run=True), a.reps)
    assert dry["keys"] == 2 * sel
    out["forget_dry_run_ms"] = round(dry_ms, 3)

    def case(ms, ms_min, **kw):
        return dict(ms=round(ms, 3), min_ms=round(ms_min, 3), slots_per_s=round(slots / (ms / 1e3)), **kw)

    # the selective question, three ways
    ms, mn, cnt = timed(lambda: be.count_keys([prefix]), a.reps)
    assert cnt["keys"] == cnt["records"] == 2 * sel and cnt["slots_scanned"] == slots
    out["selective_count_only"] = case(ms, mn, keys=cnt["keys"])
    ms, mn, (n, nb, pages) = timed(lambda: scan_pages(be, prefixes=[prefix]), a.reps)
    assert n == 2 * sel
    out["selective_scan"] = case(ms, mn, records=n, stem_bytes=nb, pages=pages)
    ms_e, mn_e, (kept, moved) = timed(lambda: export_all(be, prefix), a.export_reps)
    assert kept == 2 * sel
    out["selective_export_and_filter"] = case(ms_e, mn_e, records=kept, stem_bytes_moved=moved)
    out["selective_scan"]["speedup_over_export_and_filter"] = round(ms_e / ms, 1)

    # everything
    ms, mn, (n, nb, pages) = timed(lambda: scan_pages(be, page_records=a.page_records,
                                                      page_stem_bytes=64 * a.page_records), a.export_reps)
    assert n == info["live_slots"]
    out["list_all_scan"] = case(ms, mn, records=n, stem_bytes=nb, pages=pages, records_per_s=round(n / (ms / 1e3)))
    ms_e, mn_e, (kept, moved) = timed(lambda: export_all(be), a.export_reps)
    assert kept == n and moved == nb
    out["list_all_export"] = case(ms_e, mn_e, records=kept, records_per_s=round(kept / (ms_e / 1e3)))
    out["list_all_scan"]["speedup_over_export"] = round(ms_e / ms, 2)
    assert be.table_info() == info  # (read-only)
    be.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
