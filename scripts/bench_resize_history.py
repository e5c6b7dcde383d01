"""rl_resize_history against limiter.migrate: doubling the history log of a table
that holds C1's keys.

Fills a C1-shaped table as bench_resize.py does (tenants x {SECOND, MINUTE}
keys, BASELINE C1: 10M tenants in 2^27 slots; a second pass one window later
gives every SECOND key a history-log entry, so the call has chains to copy),
then times, with the host clock around calls that return synchronised:

  * rl_table_info_get: one read of 64 B per slot, for scale;
  * rl_resize to the same size (a full rehash of the same table), for scale;
  * limiter.migrate of the table into a second ctx whose log is twice as large
    (the only way to resize the log before rl_resize_history: every record
    through host memory), on the table as filled;
  * rl_resize_history to twice the log, back to the size it had, and once more
    to the same size, on the same ctx: one warm round, then --rounds timed ones;
    "ms" is the median, "all_ms" every timed call.

    python scripts/bench_resize_history.py [--tenants N] [--slots-log2 K] [--history-log2 H] [--rounds R] [--out FILE]

Prints one JSON line (and writes it to --out). The figure to beat is migrate_s
of the same run (migrate_new_ctx_s, creating the second ctx, comes on top of
it). The call allocates its new log inside the timed call. Under `rocprofv3
--kernel-trace --stats` (with --no-migrate, a run of its own) the kernels
k_relog_place and k_relog_commit give the device side.
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
from ratelimit_amd.limiter import Backend, migrate  # noqa: E402


def fill(be, tenants, batch, now):
    t0 = time.perf_counter()
    for lo in range(0, tenants, batch):
        be.do_limit_arrays(*W.c1_batch(np.arange(lo, min(lo + batch, tenants)), now))
    return time.perf_counter() - t0


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=10_000_000)
    ap.add_argument("--slots-log2", type=int, default=27)
    ap.add_argument("--history-log2", type=int, default=25, help="the log's entries at creation")
    ap.add_argument("--batch", type=int, default=500_000, help="requests per fill batch")
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds of the three calls, after one warm round")
    ap.add_argument("--no-migrate", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, H = 1 << a.slots_log2, 1 << a.history_log2
    kw = dict(max_batch=1 << 20, max_rules=8, hash_seed=1, jitter=2)
    be = Backend(0.8, False, table_slots=S, history_entries=H, **kw)
    fill_s = fill(be, a.tenants, a.batch, W.NOW0) + fill(be, a.tenants, a.batch, W.NOW0 + 1)
    be.table_info()  # (warm)
    info_s, info = timed(be.table_info)
    H = info["history_entries"]  # (as rounded)
    out = {"table_slots": S, "tenants": a.tenants, "keys": info["live_slots"], "history_slots": info["history_slots"],
           "history_entries": H, "history_appended": info["history_appended"], "fill_s": round(fill_s, 2),
           "table_info_ms": round(info_s * 1e3, 3)}
    be.resize(S)  # (warm)
    out["resize_same_size_ms"] = round(timed(lambda: be.resize(S))[0] * 1e3, 3)
    if not a.no_migrate:
        new_s, dst = timed(lambda: Backend(0.8, False, table_slots=S, history_entries=2 * H, **kw))
        mig_s, tot = timed(lambda: migrate(be, dst))
        assert tot["keys"] == info["live_slots"] == dst.table_info()["live_slots"]
        out.update(migrate_s=round(mig_s, 3), migrate_records=tot["records"], migrate_new_ctx_s=round(new_s, 3))
        dst.close()
    calls = (("grow_x2", 2 * H), ("shrink_back", H), ("same_size", H))
    for rnd in range(max(a.rounds, 1) + 1):
        for name, entries in calls:
            s, r = timed(lambda: be.resize_history(entries))
            assert r["chains"] == info["history_slots"] and r["entries_after"] == entries and r["chains_lost"] == 0
            if rnd == 0:  # (the warm round: its info is the one that shows what the fill left)
                out["history_" + name] = dict(r, all_ms=[])
            else:
                out["history_" + name]["all_ms"].append(round(s * 1e3, 3))
    for name, _ in calls:
        out["history_" + name]["ms"] = round(statistics.median(out["history_" + name]["all_ms"]), 3)
    after = be.table_info()
    assert all(after[k] == info[k] for k in ("live_slots", "exact_stems", "history_slots", "history_appended"))
    if not a.no_migrate:
        out["migrate_over_resize_history"] = round(out["migrate_s"] * 1e3 / out["history_grow_x2"]["ms"], 1)
    be.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
