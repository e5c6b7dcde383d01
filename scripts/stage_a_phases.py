"""Where k_part and k_bucket spend their time, phase by phase, on C1-shaped
batches: the per-tile / per-bucket stamps of a profiling build of the library
(RL_BK_PROF), read back through rl_debug_stage_a_prof after each batch.

    python -c "from ratelimit_amd import build as B; \
               B.build(out='build_abl/lib_prof.so', defines=['RL_BK_PROF=1'])"
    RL_LIB_PATH=$PWD/build_abl/lib_prof.so python scripts/stage_a_phases.py [batches=4] [out.txt]

A stamp is thread 0's clock once its wave's loads in flight have landed; the
phases of one workgroup are separated by barriers, so the differences are the
workgroup's. Per phase: the median and the 90th percentile over the workgroups
of every batch but the first, in microseconds, and per kernel the span from the
first workgroup's start to the last one's end. The stamps cost each workgroup
a few stores and waits: the spans are a little longer than the product
library's kernels.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ratelimit_amd import _lib, workloads as W  # noqa: E402
from ratelimit_amd.limiter import Backend  # noqa: E402

PART_DIGITS, MAX_PART_TILES, PART_TILE = 1024, 2048, 4096
BK_PHASES = [("setup", 0, 1), ("gather", 1, 2), ("hash / dedup", 2, 6), ("compact / reserve", 6, 8),
             ("sort / write", 8, 3), ("segment", 3, 5), ("whole workgroup", 0, 5)]
PART_PHASES = [("load", 0, 1), ("rank (multisplit)", 1, 2), ("offsets / info", 2, 3), ("LDS scatter", 3, 4),
               ("write", 4, 5), ("whole workgroup", 0, 5)]


def main():
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
    L = _lib.lib()
    if not hasattr(L, "rl_debug_stage_a_prof"):
        sys.exit("%s is not a profiling build (RL_BK_PROF)" % _lib.LIB_PATH)
    tick_us = 0.01  # the constant-rate clock: 100 MHz
    bk = np.zeros(PART_DIGITS * 16, np.uint64)
    pt = np.zeros(MAX_PART_TILES * 8, np.uint64)
    rng = np.random.default_rng(0xC1)
    be = Backend(0.8, True, table_slots=1 << 24, max_batch=1 << 20, max_rules=8, device=0)
    bks, pts = [], []
    try:
        for k in range(batches + 1):
            a, n, nq, nr = W.c1_batch(rng.integers(0, 10_000_000, 500_000), W.NOW0 + k)
            be.do_limit_arrays(a, n, nq, nr)
            rc = L.rl_debug_stage_a_prof(bk.ctypes.data_as(C.c_void_p), pt.ctypes.data_as(C.c_void_p))
            assert rc == 0
            if k:  # (the first batch: cold caches, first launches)
                bks.append(bk.reshape(PART_DIGITS, 16).astype(np.int64))
                pts.append(pt.reshape(MAX_PART_TILES, 8)[:(n + PART_TILE - 1) // PART_TILE].astype(np.int64))
    finally:
        be.close()

    def table(name, stamps, phases):
        lines = ["%s: %d workgroups x %d batches" % (name, stamps[0].shape[0], len(stamps)),
                 "  %-22s %10s %10s" % ("phase", "median us", "p90 us")]
        for label, a, b in phases:
            d = np.concatenate([(s[:, b] - s[:, a])[(s[:, b] >= s[:, a]) & (s[:, a] >= s[:, 0])] for s in stamps])
            lines.append("  %-22s %10.2f %10.2f" % (label, np.median(d) * tick_us, np.percentile(d, 90) * tick_us))
        span = [(s[:, 5].max() - s[:, 0].min()) * tick_us for s in stamps]
        lines.append("  %-22s %10.2f   (first start to last end, median over batches)" % ("kernel span",
                                                                                         float(np.median(span))))
        return lines

    text = "\n".join(table("k_part", pts, PART_PHASES) + [""] + table("k_bucket", bks, BK_PHASES))
    print(text)
    if out:
        out.write(text + "\n")


if __name__ == "__main__":
    main()
