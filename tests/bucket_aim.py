"""Aiming descriptors at one partition bucket, and a model of the route a large
bucket takes through k_big_count / k_big_place / k_bucket_big (no GPU).

Stage A sorts a batch by the top 10 bits of each stem's 32-bit sort key (the
high word of the keyed stem hash, k_prepare: keys[i] = h >> 32). Under a fixed
rl_config.hash_seed the hash is a function of the stem bytes alone, so this
module restates it (SipHash-1-3 under hash_key_of(seed), rl_device.h), hashes
candidate stems b"aim_%010d_x" and keeps those of the wanted bucket. A bucket's
positions are its descriptors in arrival order (k_part is a stable partition
per tile and bucket_src walks the tiles in order), so a test that chooses the
arrival order chooses what sample_heavy and bucket_peel see.

tools/bucket_mix.py imports hash_key and stem_hash from here, and
scripts/big_bucket_routes.py the compositions: keep those names.

Three parts: the hash (scalar and numpy) with the stem finder; the route model
(sample positions, thresholds, chunk counts); the compositions of
tests/test_gpu_big_bucket_paths.py with their batch builder.
"""
import functools

import numpy as np

# --------------------------------------------------------------------------- the stem hash
M = (1 << 64) - 1


def rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M


def fmix(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M
    return k ^ (k >> 33)


def hash_key(seed):
    """hash_key_of(seed) -> (k0, k1)."""
    return fmix(seed ^ 0x243F6A8885A308D3), fmix((seed + 0x13198A2E03707344) & M)


_IV = (0x736f6d6570736575, 0x646f72616e646f6d, 0x6c7967656e657261, 0x7465646279746573)


def stem_hash(key, s):
    """The 64-bit stem hash of bytes s, one stem at a time (plain integers)."""
    k0, k1 = key
    v = [k0 ^ _IV[0], k1 ^ _IV[1], k0 ^ _IV[2], k1 ^ _IV[3]]

    def rnd():
        v[0] = (v[0] + v[1]) & M; v[1] = rotl(v[1], 13); v[1] ^= v[0]; v[0] = rotl(v[0], 32)
        v[2] = (v[2] + v[3]) & M; v[3] = rotl(v[3], 16); v[3] ^= v[2]
        v[0] = (v[0] + v[3]) & M; v[3] = rotl(v[3], 21); v[3] ^= v[0]
        v[2] = (v[2] + v[1]) & M; v[1] = rotl(v[1], 17); v[1] ^= v[2]; v[2] = rotl(v[2], 32)

    def word(m):
        v[3] ^= m
        rnd()
        v[0] ^= m

    n, i = len(s), 0
    while i + 8 <= n:
        word(int.from_bytes(s[i:i + 8], "little"))
        i += 8
    word(((n << 56) & M) | (int.from_bytes(s[i:], "little") if i < n else 0))
    v[2] ^= 0xff
    rnd(); rnd(); rnd()
    return (v[0] ^ v[1] ^ v[2] ^ v[3]) or 1


def stem_hash_np(key, stems):
    """The same hash of n stems of one length: stems uint8[n, L] -> uint64[n]."""
    stems = np.ascontiguousarray(stems, np.uint8)
    n, L = stems.shape
    U = np.uint64
    k0, k1 = key
    v = [np.full(n, k ^ c, U) for k, c in zip((k0, k1, k0, k1), _IV)]

    def rot(x, r):
        return (x << U(r)) | (x >> U(64 - r))

    def rnd():
        v[0] = v[0] + v[1]; v[1] = rot(v[1], 13); v[1] = v[1] ^ v[0]; v[0] = rot(v[0], 32)
        v[2] = v[2] + v[3]; v[3] = rot(v[3], 16); v[3] = v[3] ^ v[2]
        v[0] = v[0] + v[3]; v[3] = rot(v[3], 21); v[3] = v[3] ^ v[0]
        v[2] = v[2] + v[1]; v[1] = rot(v[1], 17); v[1] = v[1] ^ v[2]; v[2] = rot(v[2], 32)

    def word(m):
        v[3] = v[3] ^ m
        rnd()
        v[0] = v[0] ^ m

    full = L // 8
    for i in range(full):
        word(np.ascontiguousarray(stems[:, 8 * i:8 * i + 8]).view("<u8")[:, 0])
    tail = np.zeros((n, 8), np.uint8)
    tail[:, :L - 8 * full] = stems[:, 8 * full:]
    tail[:, 7] = L & 0xFF  # (len << 56: the tail is at most 7 bytes)
    word(tail.view("<u8")[:, 0])
    v[2] = v[2] ^ U(0xff)
    rnd(); rnd(); rnd()
    h = v[0] ^ v[1] ^ v[2] ^ v[3]
    return np.where(h == 0, U(1), h)


# --------------------------------------------------------------------------- the stem finder
PART_BITS, PART_DIGITS = 10, 1024
CANDIDATES = 1 << 23
_PREFIX, _WIDTH, _SUFFIX = b"aim_", 10, b"_x"
STEM_LEN = len(_PREFIX) + _WIDTH + len(_SUFFIX)


def aim_stems(ids):
    """b"aim_%010d_x" % id for every id -> uint8[n, STEM_LEN]."""
    ids = np.asarray(ids, np.int64)
    rec = np.empty((ids.size, STEM_LEN), np.uint8)
    rec[:, :len(_PREFIX)] = np.frombuffer(_PREFIX, np.uint8)
    v = ids.copy()
    for k in range(_WIDTH - 1, -1, -1):
        rec[:, len(_PREFIX) + k] = (v % 10) + 48
        v //= 10
    rec[:, len(_PREFIX) + _WIDTH:] = np.frombuffer(_SUFFIX, np.uint8)
    return rec


def sort_keys(seed, ids):
    """The 32-bit sort keys (hash >> 32) of the aim stems of ids."""
    return (stem_hash_np(hash_key(seed), aim_stems(ids)) >> np.uint64(32)).astype(np.uint32)


_CHUNK = 1 << 19


@functools.lru_cache(maxsize=None)
def _sort_keys_chunk(seed, c):
    return sort_keys(seed, np.arange(c * _CHUNK, (c + 1) * _CHUNK))


@functools.lru_cache(maxsize=None)
def _sort_keys_upto(seed, n):
    """Sort keys of candidates [0, n), n a multiple of the chunk (each chunk hashed once)."""
    return np.concatenate([_sort_keys_chunk(seed, c) for c in range(n // _CHUNK)])


def find_ids(seed, d, want, limit=CANDIDATES):
    """The first `want` candidate ids below `limit` whose sort key falls in
    bucket d (about limit / 1024 exist), each with a sort key of its own
    (a second stem on one sort key is left out) -> (ids, sort keys)."""
    n = min(limit, 1 << 21)
    while True:
        sk = _sort_keys_upto(seed, n)
        ids = np.nonzero((sk >> np.uint32(32 - PART_BITS)) == d)[0]
        _, first = np.unique(sk[ids], return_index=True)
        ids = ids[np.sort(first)]
        if ids.size >= want or n >= limit:
            break
        n = min(2 * n, limit)
    if ids.size < want:
        raise ValueError("bucket %d has %d stems among %d candidates under seed %d, %d wanted"
                         % (d, ids.size, limit, seed, want))
    ids = ids[:want]
    return ids, sk[ids]


def background_ids(seed, avoid, count):
    """The first `count` candidate ids outside the buckets `avoid`."""
    sk = _sort_keys_upto(seed, 1 << 19)
    ids = np.nonzero(~np.isin(sk >> np.uint32(32 - PART_BITS), list(avoid)))[0]
    return ids[:count]


# --------------------------------------------------------------------------- the route model
# (rl_kernels.hip / rl_kernels.h; tests/test_bucket_aim_cpu.py compares them with the source text)
BK_HEAVY_MIN = 3            # a sampled key seen this often is heavy
BK_SAMPLES_PER_LANE = 4     # sample_heavy: 64 lanes x 4 positions
BIG_HEAVY = 4               # heavy keys kept per bucket
BK_SMALL = (4, 8)           # BkShape<waves, items>: k_bucket
BK_BIG = (8, 8)             # k_bucket_big
BK_GRID = 512               # k_bucket<LIST, true>: workgroup b walks buckets b, b + 512
SMALL_CAP = 64 * BK_SMALL[0] * BK_SMALL[1]   # 2048: a larger bucket is queued; BIG_CHUNK
BIG_CAP = 64 * BK_BIG[0] * BK_BIG[1]         # 4096: BIG_LIGHT_CAP, bucket_peel's and bucket_lsd's chunk


def kbucket_positions(S):
    """sample_heavy's 256 positions in a bucket of S."""
    ns = 64 * BK_SAMPLES_PER_LANE
    return np.array([((2 * g + 1) * S) // (2 * ns) for g in range(ns)], np.int64)


def peel_positions(S):
    """bucket_peel's 64 positions."""
    return np.array([((2 * l + 1) * S) >> 7 for l in range(64)], np.int64)


def _heavy(keys, pos):
    """Keys seen at least BK_HEAVY_MIN times at pos, ranked by first sample, the first BIG_HEAVY."""
    s = keys[pos]
    out = []
    for i, k in enumerate(s.tolist()):
        if k not in out and (s[:i] != k).all() and int((s == k).sum()) >= BK_HEAVY_MIN:
            out.append(k)
    return out[:BIG_HEAVY]


def route(keys):
    """The route of a bucket whose sort keys, in arrival order, are `keys`.

    -> dict: route ("small", "P1", "P2-peel", "P2-lsd", "P3", "P4"), S, r and
    heavy (k_bucket's), NL, chunks (k_big_count's work items), and for the
    fallback peel_r, peel_nl and lsd_chunks."""
    keys = np.asarray(keys, np.uint32)
    S = keys.size
    if S <= SMALL_CAP:
        return dict(route="small", S=S)
    heavy = _heavy(keys, kbucket_positions(S))
    r = len(heavy)
    NL = int((~np.isin(keys, heavy)).sum()) if r else 0
    out = dict(S=S, r=r, heavy=heavy, NL=NL, chunks=-(-S // SMALL_CAP) if r else 0)
    if r and NL <= BIG_CAP:
        out["route"] = "P1"
        return out
    ph = _heavy(keys, peel_positions(S))
    nl = int((~np.isin(keys, ph)).sum())
    out.update(peel_r=len(ph), peel_heavy=ph, peel_nl=nl, lsd_chunks=-(-S // BIG_CAP))
    peeled = len(ph) >= 1 and nl <= BIG_CAP
    out["route"] = ("P2-peel" if peeled else "P2-lsd") if r else ("P3" if peeled else "P4")
    return out


# --------------------------------------------------------------------------- compositions
SEED = 20260101       # rl_config.hash_seed of the aimed ctx
D_STAR = 333          # the aimed bucket; #11's second one is D_STAR ^ 512, walked by the same workgroup
NOW0 = 1_700_000_000  # (workloads.NOW0; NOW0 % 60 == 20: NOW0 + 1 rolls the second windows only)
BACKGROUND = 300


def _place_peel_only(S, rng):
    """#8: the hot key (slot 0) on all of bucket_peel's positions and never on one of k_bucket's."""
    return {0: peel_positions(S)}, {0: kbucket_positions(S)}


def _place_on_kbucket(S, rng):
    """#8 mutated: the hot key on k_bucket's positions as well."""
    return {0: np.r_[peel_positions(S), kbucket_positions(S)[::8]]}, {}


def _place_second_off_kbucket(S, rng):
    """#9: the second hot key (slot 1) off all of k_bucket's positions, on eight of bucket_peel's."""
    kb = kbucket_positions(S)
    pp = peel_positions(S)
    return {1: pp[~np.isin(pp, kb)][::7][:8]}, {1: kb}


# name -> hot (descriptors per hot key), L (light descriptors), pairs (light stems
# used twice), place, and what the model must say: route, NL, chunks, lsd_chunks
SPECS = {
    "1": dict(hot=(2049,), L=0, route="P1", NL=0, chunks=2),
    "2": dict(hot=(1500, 1200), L=1396, route="P1", NL=1396, chunks=2),
    "3": dict(hot=(900, 800, 700), L=1697, route="P1", NL=1697, chunks=3),
    "4": dict(hot=(800,) * 4, L=4096, route="P1", NL=4096, chunks=4),
    "5": dict(hot=(800,) * 4, L=4097, route="P2-lsd", NL=4097, chunks=4, lsd_chunks=2, peel_nl=4097),
    "5p": dict(hot=(800,) * 4, L=4097, pairs=True, route="P2-lsd", NL=4097, chunks=4, lsd_chunks=2, peel_nl=4097),
    "6": dict(hot=(1000,) * 6, L=100, route="P1", NL=2100, chunks=3),
    "7": dict(hot=(1100,) * 9, L=0, route="P2-lsd", NL=5500, chunks=5, lsd_chunks=3),
    "8": dict(hot=(1100,), L=4020, place=_place_peel_only, route="P3", lsd_chunks=2, peel_nl=4020),
    "9": dict(hot=(3000, 3000), L=1500, place=_place_second_off_kbucket, route="P2-peel", NL=4500, chunks=4,
              peel_nl=1500),
    "10": dict(hot=(), L=4200, route="P4", lsd_chunks=2),
    "10p": dict(hot=(), L=4200, pairs=True, route="P4", lsd_chunks=2),
}
# composition -> its aimed buckets
COMPOSITIONS = {k: ((D_STAR, k),) for k in SPECS}
COMPOSITIONS["11"] = ((D_STAR, "2"), (D_STAR ^ BK_GRID, "5"))


def spec(name, **change):
    s = dict(pairs=False, place=None)
    s.update(SPECS[name])
    s.update(change)
    return s


def bucket_slots(sp, rng):
    """One bucket's arrival order as stem slots: hot key c is slot c, the light
    stems are slots r, r + 1, ... (each once, or twice with pairs)."""
    hot, L, r = sp["hot"], sp["L"], len(sp["hot"])
    S = sum(hot) + L
    light = r + (np.arange(L) // 2 if sp["pairs"] else np.arange(L))
    left = [np.full(c, k) for k, c in enumerate(hot)]
    seq = np.full(S, -1, np.int64)
    must, forbid = sp["place"](S, rng) if sp["place"] else ({}, {})
    for k, pos in must.items():
        pos = np.unique(pos)
        seq[pos] = k
        left[k] = left[k][pos.size:]
    for k, pos in forbid.items():  # the rest of a constrained key: anywhere else
        free = np.nonzero(seq < 0)[0]
        free = rng.permutation(free[~np.isin(free, pos)])[:left[k].size]
        seq[free] = k
        left[k] = left[k][:0]
    rest = rng.permutation(np.concatenate(left + [light]).astype(np.int64))
    seq[seq < 0] = rest
    return seq


class Aimed:
    """One composition under a hash seed: the batch arrays (one descriptor per
    request) and, per aimed bucket, its sort keys in arrival order."""

    def __init__(self, name, seed=SEED, **change):
        self.name, self.seed = name, seed
        rng = np.random.default_rng([seed, sum(name.encode()), len(name)])
        parts, self.buckets = [], []
        for d, sname in COMPOSITIONS[name]:
            sp = spec(sname, **change)
            slots = bucket_slots(sp, rng)
            ids, sk = find_ids(seed, d, int(slots.max()) + 1)
            self.buckets.append(dict(d=d, spec=sp, slots=slots, ids=ids, keys=sk[slots], n_hot=len(sp["hot"])))
            parts.append(ids[slots])
        bg = background_ids(seed, [d for d, _ in COMPOSITIONS[name]], BACKGROUND)
        parts.append(np.r_[bg, bg[:BACKGROUND // 4]][rng.permutation(BACKGROUND + BACKGROUND // 4)])
        # arrival order: the parts interleaved at random, each part's own order kept
        label = rng.permutation(np.concatenate([np.full(p.size, i) for i, p in enumerate(parts)]))
        self.ids = np.empty(label.size, np.int64)
        for i, p in enumerate(parts):
            self.ids[label == i] = p
        n = self.n = self.ids.size
        self.hits = rng.integers(0, 9, n).astype(np.uint32)
        # per stem: unit SECOND / MINUTE by its id, and a limit its descriptors
        # cross inside one batch where it has enough of them: a hot key's at
        # 30 .. 90 % of its hits, a light stem's at 1 .. 12
        uniq, inv, cnt = np.unique(self.ids, return_inverse=True, return_counts=True)
        tot = np.bincount(inv, np.maximum(self.hits, 1)).astype(np.int64)
        lim = np.where(cnt > 4, tot * (3 + 2 * (uniq % 4)) // 10, 1 + uniq % 12)
        self.unit = (1 + (self.ids & 1)).astype(np.uint8)
        self.limit = np.maximum(lim[inv], 1).astype(np.uint32)
        self.hot_total, self.hot_limit = tot[cnt > 4], lim[cnt > 4]

    def batch(self, now):
        n = self.n
        return {
            "stem_bytes": aim_stems(self.ids).reshape(-1),
            "stem_off": (np.arange(n + 1, dtype=np.uint64) * STEM_LEN).astype(np.uint32),
            "now": np.full(n, now, np.int64),
            "req_idx": np.arange(n, dtype=np.uint32),
            "unit": self.unit.copy(),
            "flags": np.zeros(n, np.uint8),
            "limit": self.limit.copy(),
            "hits": self.hits.copy(),
            "rule_id": (self.unit - 1).astype(np.uint32),
        }, n, n, 2

    def batches(self):
        """Three batches of the composition: two in one second, one in the next."""
        return [self.batch(NOW0), self.batch(NOW0), self.batch(NOW0 + 1)]

    def routes(self):
        return [route(b["keys"]) for b in self.buckets]


@functools.lru_cache(maxsize=None)
def aimed(name):
    return Aimed(name)
