"""rl_resize against limiter.migrate: doubling a table that holds C1's keys.

Fills a C1-shaped table (tenants x {SECOND, MINUTE} keys, BASELINE C1: 10M
tenants in 2^27 slots; a second pass one window later gives every SECOND key a
history-log entry, so the re-link has work), then times, with the host clock
around calls that return synchronised:

  * rl_table_info_get: one read of the same 64 B per slot, for scale;
  * limiter.migrate of the table into a second ctx of twice the slots (the
    only way to grow before rl_resize: every record through host memory), on
    the table as filled;
  * rl_resize to twice the slots, back to the size it had, and once more to
    the same size (each on the same ctx, which keeps serving), --rounds times
    over: "ms" is the first round's call, "all_ms" every round's.

    python scripts/bench_resize.py [--tenants N] [--slots-log2 K] [--rounds R] [--out FILE]

Prints one JSON line (and writes it to --out). The figure to beat is
migrate_s of the same run (migrate_new_ctx_s, creating the second ctx, comes on
top of it). A resize allocates its new table inside the timed call: where the
runtime has to fetch gigabytes from the driver, that allocation is most of it
(all_ms shows both kinds of call). Under `rocprofv3 --kernel-trace --stats` the kernels
k_resize_place and k_resize_relink give the device side.
"""
import argparse
import json
import os
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
    ap.add_argument("--batch", type=int, default=500_000, help="requests per fill batch")
    ap.add_argument("--rounds", type=int, default=3, help="times the three resizes are repeated")
    ap.add_argument("--no-migrate", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S = 1 << a.slots_log2
    kw = dict(max_batch=1 << 20, max_rules=8, hash_seed=1, jitter=2, history_entries=1 << 25)
    be = Backend(0.8, False, table_slots=S, **kw)
    fill_s = fill(be, a.tenants, a.batch, W.NOW0) + fill(be, a.tenants, a.batch, W.NOW0 + 1)
    be.table_info()  # (warm)
    info_s, info = timed(be.table_info)
    out = {"table_slots": S, "tenants": a.tenants, "keys": info["live_slots"], "history_slots": info["history_slots"],
           "fill_s": round(fill_s, 2), "table_info_ms": round(info_s * 1e3, 3)}
    if not a.no_migrate:
        new_s, dst = timed(lambda: Backend(0.8, False, table_slots=2 * S, **kw))
        mig_s, tot = timed(lambda: migrate(be, dst))
        assert tot["keys"] == info["live_slots"] == dst.table_info()["live_slots"]
        out.update(migrate_s=round(mig_s, 3), migrate_records=tot["records"], migrate_new_ctx_s=round(new_s, 3))
        dst.close()
    for rnd in range(max(a.rounds, 1)):
        for name, slots in (("grow_x2", 2 * S), ("shrink_back", S), ("same_size", S)):
            s, r = timed(lambda: be.resize(slots))
            assert r["keys"] == info["live_slots"] and r["slots_after"] == slots
            if rnd == 0:
                out["resize_" + name] = dict(r, ms=round(s * 1e3, 3), all_ms=[])
            out["resize_" + name]["all_ms"].append(round(s * 1e3, 3))
    after = be.table_info()
    assert all(after[k] == info[k] for k in ("live_slots", "exact_stems", "history_slots", "history_appended"))
    if not a.no_migrate:
        out["migrate_over_resize"] = round(out["migrate_s"] * 1e3 / out["resize_grow_x2"]["ms"], 1)
    be.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
