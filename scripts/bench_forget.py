"""rl_forget against its nearest yardsticks: fills a C1-shaped table (tenants x
{SECOND, MINUTE} keys, BASELINE C1: 10M tenants in 2^27 slots = 20M keys) through
the workload generators, then times, with the host clock around synchronous calls
on the same table in one process:

  * the scans it is compared with: rl_table_info_get (64 B per slot) and
    rl_hot_keys with k = 10 (k_hot_scan: the slots' first 32 bytes, as
    k_forget_scan reads them);
  * one prefix scan (RL_FORGET_PREFIX | RL_FORGET_DRY_RUN, so that it can be
    repeated: the same loads and comparisons, no stores) for 1 and for 64
    prefixes, each with prefixes no stem begins with (one set that differs from
    every stem in its first 4 bytes, which the filter on the slot's first 32
    bytes rejects, and one that shares the stems' first 14 bytes) and with a
    prefix that selects about 1 % of the keys (tenants 0..99999; among 64
    prefixes it is the last); then that 1 % deleted for real, once;
  * keyed deletion of --keys present stems (the MINUTE stems of tenants drawn
    without replacement, another set each rep), after rl_lookup of the same
    stems: both the C call alone on prebuilt arrays.

    python scripts/bench_forget.py [--tenants N] [--slots-log2 K] [--keys N] [--reps R]

Prints one JSON line. Scan figures are the median of R calls after a warm one,
keyed figures the best of R. Under `rocprofv3 --kernel-trace --stats` the kernels
k_forget_scan, k_forget_keys, k_hot_scan, k_lookup and k_table_info give the
device side.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ratelimit_amd import abi, workloads as W  # noqa: E402
from ratelimit_amd.limiter import Backend  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=10_000_000)
    ap.add_argument("--slots-log2", type=int, default=27)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=500_000, help="requests per fill batch")
    return ap.parse_args(argv)


def prefix_sets(tenants):
    """{case: (prefixes, tenants whose two keys they select)}."""
    one_pct = min(100_000, tenants)
    hot = b"bench_tenant_t00000" if tenants > 100_000 else b"bench_tenant_t"
    miss_head = [b"zz%02d_other_domain_" % j for j in range(64)]
    miss_shared = [b"bench_tenant_t9%02d" % j for j in range(64)]
    return {
        "1_selective": (miss_head[:1], 0), "1_selective_shared_head": (miss_shared[:1], 0), "1_one_percent": ([hot], one_pct),
        "64_selective": (miss_head, 0), "64_selective_shared_head": (miss_shared, 0),
        "64_one_percent": (miss_shared[:63] + [hot], one_pct),
    }


def timed(f, reps):
    f()  # (warm)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, min(ts) * 1e3, r


def main():
    a = parse_args()
    cap = 1 << 20
    n = min(a.keys, cap, a.tenants // max(a.reps, 1))
    slots = 1 << a.slots_log2
    be = Backend(0.8, False, table_slots=slots, max_batch=cap, max_rules=8, hash_seed=1)
    t0 = time.perf_counter()
    for lo in range(0, a.tenants, a.batch):
        be.do_limit_arrays(*W.c1_batch(np.arange(lo, min(lo + a.batch, a.tenants)), W.NOW0))
    out = {"table_slots": slots, "tenants": a.tenants, "reps": a.reps, "fill_s": round(time.perf_counter() - t0, 2)}

    info_ms, _, info = timed(be.table_info, a.reps)
    hot_ms, _, _ = timed(lambda: be.hot_keys(W.NOW0, 10), a.reps)
    out.update(keys=info["live_slots"], table_info_ms=round(info_ms, 3), hot_keys_k10_ms=round(hot_ms, 3))

    out["prefix_scan"] = {}
    for case, (prefixes, sel) in prefix_sets(a.tenants).items():
        ms, ms_min, r = timed(lambda: be.forget(prefixes, prefix=True, dry_run=True), a.reps)
        assert r["keys"] == 2 * sel and r["slots_scanned"] == slots, (case, r)
        out["prefix_scan"][case] = {"ms": round(ms, 3), "min_ms": round(ms_min, 3), "slots_per_s": round(slots / (ms / 1e3)),
                                    "ratio_to_hot_keys": round(ms / hot_ms, 2), "keys": r["keys"]}

    # keyed: rl_lookup, then rl_forget, of the same present stems
    perm = np.random.default_rng(7).permutation(a.tenants)
    look_s, forget_s = [], []
    for rep in range(a.reps):
        ten = perm[rep * n:(rep + 1) * n]
        x = W.c1_batch(ten, W.NOW0)[0]
        L = int(x["stem_off"][1])
        blob = np.ascontiguousarray(x["stem_bytes"].reshape(2 * n, L)[1::2]).reshape(-1)  # the MINUTE stems
        off = (np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32)
        units, nows = np.full(n, 2, np.uint8), np.full(n, W.NOW0 + 5, np.int64)
        res = {f: np.zeros(n, dt) for f, dt in abi.KEY_STATE_DTYPES.items()}
        k, s = abi.RlKeys(), abi.RlKeyState()
        k.n = n
        k.stem_bytes, k.stem_off, k.unit, k.now = abi.ptr(blob), abi.ptr(off), abi.ptr(units), abi.ptr(nows)
        for f, v in res.items():
            setattr(s, f, abi.ptr(v))
        t0 = time.perf_counter()
        be._check(be.L.rl_lookup(be.ctx, C.byref(k), C.byref(s)))
        look_s.append(time.perf_counter() - t0)
        assert res["found"].all()
        st, removed, fi = abi.RlStems(), np.zeros(n, np.uint32), abi.RlForgetInfo()
        st.n, st.flags, st.stem_bytes, st.stem_off = n, 0, abi.ptr(blob), abi.ptr(off)
        t0 = time.perf_counter()
        be._check(be.L.rl_forget(be.ctx, C.byref(st), abi.ptr(removed), C.byref(fi)))
        forget_s.append(time.perf_counter() - t0)
        assert (removed == 1).all() and fi.keys == n
    out["keyed"] = {"keys": n, "stem_bytes": L, "lookup_s": round(min(look_s), 5), "lookup_keys_per_s": round(n / min(look_s)),
                    "forget_s": round(min(forget_s), 5), "forget_keys_per_s": round(n / min(forget_s)),
                    "forget_over_lookup_rate": round(min(look_s) / min(forget_s), 2)}

    # the 1 % deleted for real, once (some of its MINUTE keys went with the keyed reps)
    prefixes, sel = prefix_sets(a.tenants)["1_one_percent"]
    want = be.forget(prefixes, prefix=True, dry_run=True)["keys"]
    t0 = time.perf_counter()
    r = be.forget(prefixes, prefix=True)
    out["prefix_delete_one_percent"] = {"ms": round((time.perf_counter() - t0) * 1e3, 3), "keys": r["keys"]}
    assert sel <= r["keys"] == want <= 2 * sel
    after = be.table_info()
    assert after["live_slots"] == info["live_slots"] - a.reps * n - r["keys"]
    assert after["tombstones"] == a.reps * n + r["keys"]
    be.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
