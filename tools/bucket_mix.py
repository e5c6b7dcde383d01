"""Which stems share a partition bucket (top 10 bits of the 32-bit sort key)
with the hottest stems of bench.py's C2 batches, under a given stem-hash key.

The stem hash is the library's keyed SipHash-1-3 (rl_device.h StemHasher,
hash_key_of) as tests/bucket_aim.py restates it; the batches are
bench.py's four distinct C2 batches (rng 0xC2, Zipf(1.1) over 10M tenants).

    python tools/bucket_mix.py <hash_seed> [buckets=4]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ratelimit_amd import workloads as W  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from bucket_aim import hash_key, stem_hash  # noqa: E402  (the restated hash, shared with the tests)


def main():
    key = hash_key(int(sys.argv[1]))
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    rng = np.random.default_rng(0xC2)
    z = W.ZipfSampler(10_000_000, 1.1)
    for b in range(4):
        ten = z.sample(rng, 500_000)
        rng.integers(1, 9, 500_000)  # (the batch's hits, drawn by bench.py in between)
        t, c = np.unique(ten, return_counts=True)
        buckets = {}
        for tt, cc in zip(t, c):
            for suf in (b"_tier_sec_", b"_tier_min_"):
                sk = stem_hash(key, b"bench_tenant_t" + b"%010d" % tt + suf) >> 32
                buckets.setdefault(sk >> 22, []).append((int(cc), sk))
        top = sorted(((sum(x for x, _ in v), d, sorted(v, reverse=True)[:4]) for d, v in buckets.items()),
                     reverse=True)[:nb]
        for tot, d, keys in top:
            print("batch %d bucket %4d: %6d descriptors; largest stems %s" % (
                b, d, tot, ", ".join("%d (sort key %08x)" % (x, k) for x, k in keys)))


if __name__ == "__main__":
    main()
