"""Which route each composition of tests/bucket_aim.py takes through the
large-bucket kernels on the device, read from the per-bucket phase stamps of a
profiling build of the library (RL_BK_PROF, rl_debug_stage_a_prof).

    python -c "from ratelimit_amd import build as B; \
               B.build(out='build_abl/lib_prof.so', defines=['RL_BK_PROF=1'])"
    RL_LIB_PATH=$PWD/build_abl/lib_prof.so python scripts/big_bucket_routes.py [out.md]

Each composition runs once on a fresh ctx. k_bucket_big stamps 0 when it takes
a bucket, 1 when it enters the one-workgroup fallback, 13 when bucket_peel has
compacted a light part that fits, 15 when bucket_peel is done, 4 when
bucket_segment has counted the runs of a part it was given unsegmented, 7 at
the end. A stamp counts if it is newer than the bucket's stamp 0 of that batch:
neither 1 nor 13: chunk-parallel (P1); 1, 13 and 15: the fallback's peel (P3,
or P2 when k_bucket had reserved hot runs); 1 and 4 without 15: the fallback's
LSD passes (P2 or P4). The answers are compared with the C oracle's as well.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bucket_aim as A  # noqa: E402
from oracle import c_oracle  # noqa: E402
from ratelimit_amd import _lib  # noqa: E402
from ratelimit_amd.limiter import Backend  # noqa: E402

PART_DIGITS, MAX_PART_TILES = 1024, 2048
CLASS = {"P1": "chunk-parallel", "P2-peel": "fallback: peel", "P3": "fallback: peel", "P2-lsd": "fallback: LSD",
         "P4": "fallback: LSD"}


def observed(st):
    # st[0] is k_bucket_big's (it runs after k_bucket, whose bucket_one stamps 0 too, and overwrites it); the
    # stamps live in the library, not the ctx, so an earlier composition's are still there, but older than st[0].
    # A bucket k_bucket_big never took has no stamp 7 after its stamp 0 and is reported as such.
    newer = {k for k in (1, 4, 7, 13, 14, 15) if st[k] > st[0]}
    if 7 not in newer:
        return "not taken by k_bucket_big", newer
    if 1 not in newer and 13 not in newer:
        return "chunk-parallel", newer
    if {1, 13, 15} <= newer:
        return "fallback: peel", newer
    if {1, 4} <= newer and 15 not in newer:
        return "fallback: LSD", newer
    return "unclear", newer


def main():
    L = _lib.lib()
    if not hasattr(L, "rl_debug_stage_a_prof"):
        sys.exit("%s is not a profiling build (RL_BK_PROF)" % _lib.LIB_PATH)
    bk = np.zeros(PART_DIGITS * 16, np.uint64)
    pt = np.zeros(MAX_PART_TILES * 8, np.uint64)
    rows = ["| composition | bucket | S | model | stamps newer than 0 | observed | answers |",
            "|---|---|---|---|---|---|---|"]
    bad = 0
    for name in ["1", "2", "3", "4", "5", "5p", "6", "7", "8", "9", "10", "10p", "11"]:
        a = A.aimed(name)
        batch = a.batch(A.NOW0)
        co = c_oracle.COracle(0.8, False)
        want = co.do_limit(*batch)
        co.close()
        be = Backend(0.8, False, table_slots=1 << 16, max_batch=1 << 14, max_rules=8, hash_seed=A.SEED)
        try:
            got = be.do_limit_arrays(*batch)
            assert L.rl_debug_stage_a_prof(bk.ctypes.data_as(C.c_void_p), pt.ctypes.data_as(C.c_void_p)) == 0
        finally:
            be.close()
        same = all(np.array_equal(got[k], want[k]) for k in ("code", "limit_remaining", "reset_s", "stats"))
        for b, r in zip(a.buckets, a.routes()):
            obs, newer = observed(bk.reshape(PART_DIGITS, 16)[b["d"]].astype(np.int64))
            ok = obs == CLASS[r["route"]]
            bad += (not ok) + (not same)
            model = "%s (r = %d, NL = %d%s)" % (r["route"], r["r"], r["NL"], "" if r["route"] == "P1" else
                                               ", peel r = %d, nl = %d, LSD chunks %d" % (
                                                   r["peel_r"], r["peel_nl"], r["lsd_chunks"]))
            rows.append("| #%s | %d | %d | %s | %s | %s%s | %s |" % (
                name, b["d"], r["S"], model, " ".join(map(str, sorted(newer))), obs, "" if ok else " (DISAGREES)",
                "equal the oracle's" if same else "DIFFER"))
    text = "\n".join(rows)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
