"""Limits, addends, counts and clocks at the top of the u32 range: the helper
of tests/test_magnitude_cpu.py and tests/test_gpu_magnitude.py.

* ``LIMIT_EDGES`` / ``HITS_EDGES`` / ``CLOCK_EPOCHS``: the values every stream
  here draws from (around 2^24: the fp32 mantissa; around 2^31: the sign bit;
  2^32 - 1: the top), and the clocks at both ends of the accepted range.
* ``ExactModel`` / ``exact_model``: the fixed-window semantics of DESIGN.md §2
  in exact integers (Python ints, nothing masked), one counter per
  (stem bytes, windowStart) with EXPIRE. It raises ``OutOfModel`` where the Go
  code's u32 arithmetic would wrap, so a stream it accepts is one on which
  exact integers and u32 agree.
* ``scale`` and ``crossing_runs``: overwrite the values of a packed batch
  (workloads.* shapes) with edge values, inside a per-key budget, and build
  runs that cross ``near`` and the limit at a chosen element.
* ``STREAMS``: the builders of every stream the GPU file runs; the CPU file
  proves on the same objects that the model and the oracles agree.
"""
import functools
import json
import math
import os

import numpy as np

from oracle import oracle as O
from ratelimit_amd import workloads as W

U32_MAX = 2 ** 32 - 1
NOW_MAX = 0xFFFFFFFF - 2 * 86400  # rl_device.h: now + 2 * div must fit u32
LIMIT_EDGES = [0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1]
HITS_EDGES = [0, 1, 2 ** 16, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
CLOCK_EPOCHS = {"now0": W.NOW0, "zero": 0, "top": NOW_MAX - 2}
DIV = {1: 1, 2: 60, 3: 3600, 4: 86400}
OK, OVER = 1, 2
FIELDS = ("code", "limit_remaining", "reset_s", "stats")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "own_u32_edges.json")


class OutOfModel(Exception):
    """The stream left what exact integers describe: a count above 2^32 - 1, or
    a u32 subtraction of the Go code below zero."""


# --------------------------------------------------------------------------- the exact-integer model
@functools.lru_cache(maxsize=None)
def near_threshold(limit, ratio):
    """base_limiter.go:94 ``uint32(math.Floor(float64(float32(limit) * ratio)))``
    from numpy fp32: one fp32 multiply, floor."""
    near = int(math.floor(float(np.float32(limit) * np.float32(ratio))))
    if near > U32_MAX:
        # float32(limit) rounds 2^32 - 2 and 2^32 - 1 up to 2^32, and at ratio 1.0 the
        # product stays there. Go converts through int64 and keeps the low 32 bits:
        # uint32(2^32) == 0. The only conversion here that is not an identity on the
        # model's range; a larger product (ratio > 1) is outside the model.
        if near != 2 ** 32:
            raise OutOfModel("near threshold %d" % near)
        near = 0
    return near


def _sub(a, b, what):
    if a < b:
        raise OutOfModel("%s: %d - %d" % (what, a, b))
    return a - b


def decide(before, after, lc_hit, h, limit, ratio, shadow, lc_enabled):
    """GetResponseDescriptorStatus for a non-empty key (base_limiter.go:82-134)
    -> (code, remaining, deltas in O.STAT_FIELDS order, local cache set)."""
    over_limit = near_limit = lcs = within = shadow_mode = 0
    over = lc_set = False
    if lc_hit:
        over = True
        over_limit += h
        lcs += h
        code, rem = OVER, 0
    else:
        near = near_threshold(limit, ratio)
        if after > limit:
            over = True
            code, rem = OVER, 0
            if before >= limit:  # checkOverLimitThreshold, base_limiter.go:150-165
                over_limit += h
            else:
                over_limit += _sub(after, limit, "after - limit")
                near_limit += _sub(limit, max(near, before), "limit - max(near, before)")
            lc_set = bool(lc_enabled)
        else:
            code, rem = OK, _sub(limit, after, "limit - after")
            if after > near:  # checkNearLimitThreshold, base_limiter.go:167-179
                near_limit += h if before >= near else _sub(after, near, "after - near")
            within += h
    if over and shadow:
        code = OK
        shadow_mode += h
    return code, rem, (0, over_limit, near_limit, lcs, within, shadow_mode), lc_set


def stems_of(a, n):
    off = a["stem_off"]
    blob = a["stem_bytes"].tobytes()
    return [blob[int(off[i]):int(off[i + 1])] for i in range(n)]


class ExactModel:
    """fixedRateLimitCacheImpl.DoLimit (fixed_cache_impl.go:33-113) request by
    request over packed batches, in exact integers."""

    def __init__(self, ratio=0.8, local_cache=False):
        self.ratio = ratio
        self.lc_enabled = local_cache
        self.redis = {}  # (stem, windowStart) -> [count, expire]
        self.lc = {}     # (stem, windowStart) -> expireAt

    def do_limit(self, a, n, nq, nr):
        stems = stems_of(a, n)
        req, unit, flags = a["req_idx"].tolist(), a["unit"].tolist(), a["flags"].tolist()
        limit, hits, rule, nows = a["limit"].tolist(), a["hits"].tolist(), a["rule_id"].tolist(), a["now"].tolist()
        o_code, o_rem, o_reset, o_bef, o_aft, o_lc = ([0] * n for _ in range(6))
        stats = [0] * (nr * 6)
        i = 0
        while i < n:
            e = i
            while e < n and req[e] == req[i]:
                e += 1
            now = nows[req[i]]
            keys, hs, lcf, after = [], [], [], []
            for k in range(i, e):
                d = DIV[unit[k]]
                keys.append((stems[k], now // d * d))
                hs.append(max(1, hits[k]))  # fixed_cache_impl.go:41
                stats[rule[k] * 6] += hs[-1]  # TotalHits, base_limiter.go:55-57
            for j, k in enumerate(range(i, e)):  # the local cache first, for every key (:51-67)
                hit = self.lc_enabled and now < self.lc.get(keys[j], -1)
                lcf.append((2 if flags[k] & 1 else 1) if hit else 0)
            for j, k in enumerate(range(i, e)):  # INCRBY + EXPIRE (:69-95)
                if lcf[j]:
                    after.append(0)
                    continue
                ent = self.redis.get(keys[j])
                cnt = ent[0] if ent is not None and now <= ent[1] else 0
                cnt += hs[j]
                if cnt > U32_MAX:
                    raise OutOfModel("count %d of %r" % (cnt, keys[j]))
                self.redis[keys[j]] = [cnt, now + DIV[unit[k]]]
                after.append(cnt)
            for j, k in enumerate(range(i, e)):  # statuses (:100-110)
                d = DIV[unit[k]]
                if lcf[j] == 2:
                    # Q-SL (fixed_cache_impl_test.go:576-586): a shadow rule that hits the
                    # local cache skips INCRBY, so results[i] stays 0 and Go computes
                    # before = 0 - hits in u32. after = 0 is over no limit and above no
                    # near threshold, so `before` is never read: OK, remaining = limit.
                    code, rem, dl, lc_set = OK, limit[k], (0, 0, 0, 0, hs[j], 0), False
                    bef = None
                else:
                    bef = after[j] - hs[j] if not lcf[j] else None
                    code, rem, dl, lc_set = decide(bef, after[j], lcf[j] == 1, hs[j], limit[k], self.ratio,
                                                   bool(flags[k] & 1), self.lc_enabled)
                if lc_set:
                    self.lc[keys[j]] = now + d
                o_code[k], o_rem[k], o_reset[k] = code, rem, d - now % d
                o_bef[k], o_aft[k], o_lc[k] = bef, after[j], lcf[j] != 0
                for f in range(1, 6):
                    stats[rule[k] * 6 + f] += dl[f]
            i = e
        return {"code": np.array(o_code, np.uint8), "limit_remaining": np.array(o_rem, np.uint32),
                "reset_s": np.array(o_reset, np.uint32), "stats": np.array(stats, np.uint64),
                "before": o_bef, "after": o_aft, "lc_hit": np.array(o_lc, bool)}


def exact_model(batches, ratio=0.8, local_cache=False):
    m = ExactModel(ratio, local_cache)
    return [m.do_limit(a, n, nq, nr) for a, n, nq, nr in batches]


# --------------------------------------------------------------------------- the Python oracle over packed batches
def python_oracle_packed(batches, ratio=0.8, local_cache=False):
    """oracle.OracleFixedRateLimitCache over packed batches: each request
    becomes a call whose descriptors rebuild the packed stems (domain = the
    stem up to its first '_', one entry holding the rest), so the key strings
    are the packed ones. Per-rule stats are differences of the rule's counters."""
    oc = O.OracleFixedRateLimitCache(ratio, local_cache)
    rules = {}
    res = []
    for a, n, nq, nr in batches:
        stems = stems_of(a, n)
        out = {"code": np.zeros(n, np.uint8), "limit_remaining": np.zeros(n, np.uint32),
               "reset_s": np.zeros(n, np.uint32), "stats": np.zeros(nr * 6, np.uint64)}
        base = {r: st.as_tuple() for r, st in rules.items()}
        i = 0
        while i < n:
            e = i
            while e < n and a["req_idx"][e] == a["req_idx"][i]:
                e += 1
            descs, limits = [], []
            dom = stems[i].split(b"_", 1)[0]
            for k in range(i, e):
                d, rest = stems[k].split(b"_", 1)
                key, val = rest[:-1].rsplit(b"_", 1)
                assert d == dom and a["hits"][k] == a["hits"][i] and stems[k].endswith(b"_")
                descs.append(O.Descriptor([(key.decode(), val.decode())]))
                st = rules.setdefault(int(a["rule_id"][k]), O.RateLimitStats("rule%d" % a["rule_id"][k]))
                limits.append(O.RateLimit(st.key, st, O.Limit(int(a["limit"][k]), int(a["unit"][k])), False,
                                          bool(a["flags"][k] & 1)))
            now = int(a["now"][a["req_idx"][i]])
            sts = oc.do_limit(O.RateLimitRequest(dom.decode(), descs, int(a["hits"][i])), limits, now)
            for k, s in zip(range(i, e), sts):
                out["code"][k], out["limit_remaining"][k], out["reset_s"][k] = (s.code, s.limit_remaining,
                                                                                 s.duration_until_reset)
            i = e
        for r, st in rules.items():
            if r < nr:
                out["stats"][r * 6:r * 6 + 6] = [x - y for x, y in zip(st.as_tuple(), base.get(r, (0,) * 6))]
        res.append(out)
    return res, oc


# --------------------------------------------------------------------------- values
def _keys(a, n):
    stems = stems_of(a, n)
    now = a["now"][a["req_idx"][:n]].tolist()
    unit = a["unit"].tolist()
    return stems, [(s, t // DIV[u] * DIV[u]) for s, t, u in zip(stems, now, unit)]


def account(a, n, running, requests=None):
    """Add the batch's max(1, hits) to the running per-(stem, window) sums and
    keep its limits for the stream (``requests``: a mask, default all)."""
    used, lim = running.setdefault("used", {}), running.setdefault("limit", {})
    stems, keys = _keys(a, n)
    req, rule, hits, limit = a["req_idx"].tolist(), a["rule_id"].tolist(), a["hits"].tolist(), a["limit"].tolist()
    for k in range(n):
        if requests is not None and not requests[req[k]]:
            continue
        used[keys[k]] = used.get(keys[k], 0) + max(1, hits[k])
        lim.setdefault((stems[k], rule[k]), limit[k])
        running.setdefault("shadow", {}).setdefault(stems[k], bool(a["flags"][k] & 1))
        if used[keys[k]] > running.get("budget", U32_MAX):
            raise OutOfModel("budget: %d for %r" % (used[keys[k]], keys[k]))


def scale(a, n, rng, limits, hits, budget=U32_MAX, running=None, reserve=1024, requests=None, p_shadow=0.0):
    """Overwrite a["limit"] and a["hits"] of a packed batch with draws from the
    edge sets. A limit is drawn once per (stem, rule) and kept for the stream;
    hits are drawn per request (``hits``: a list to choose from, or a callable
    rng -> int) and clipped so that the sum of max(1, hits) per (stem, window)
    stays <= budget over the whole stream (``running``: the dict carried from
    batch to batch). ``reserve`` keeps that much of a key's budget back for
    later hits of 1; a key with no room left raises. ``requests``: a boolean
    mask of the requests to touch (default all). ``p_shadow``: the share of
    stems whose descriptors are flagged shadow_mode (drawn once per stem)."""
    running = {} if running is None else running
    running["budget"] = budget
    used, lim = running.setdefault("used", {}), running.setdefault("limit", {})
    shadow = running.setdefault("shadow", {})
    stems, keys = _keys(a, n)
    req, rule = a["req_idx"].tolist(), a["rule_id"].tolist()
    i = 0
    while i < n:
        e = i
        while e < n and req[e] == req[i]:
            e += 1
        if requests is None or requests[req[i]]:
            h = int(hits(rng)) if callable(hits) else int(hits[rng.integers(len(hits))])
            room = min((budget - used.get(k, 0)) // keys[i:e].count(k) for k in keys[i:e])  # (a key twice: twice h)
            if room < 1:
                raise OutOfModel("no room left for %r" % (keys[i:e],))
            h = min(h, max(room - reserve, 1))
            for k in range(i, e):
                a["hits"][k] = h
                used[keys[k]] = used.get(keys[k], 0) + max(1, h)
                lk = (stems[k], rule[k])
                if lk not in lim:
                    lim[lk] = int(limits[rng.integers(len(limits))])
                a["limit"][k] = lim[lk]
                if p_shadow:
                    if stems[k] not in shadow:
                        shadow[stems[k]] = bool(rng.random() < p_shadow)
                    a["flags"][k] = 1 if shadow[stems[k]] else 0
        i = e
    return running


def crossing_runs(ten, hot, now, rng, limits, cross_at=("first", "mid", "last"), ratio=0.8, top=2 ** 32 - 4096):
    """Two C1-shaped batches in which every tenant of ``hot`` crosses its near
    threshold and its limit inside batch 2, at a chosen element of its run.

    ``ten``: the tenants of batch 2 in arrival order (hot tenants as runs of any
    length, the rest untouched: hits 1 and c1_batch's limits, for ``scale``).
    Tenant hot[i] gets the limit L = limits[i % len] (2^32 - 1 and 2^32 - 2
    cannot be crossed with room for the run's later elements below 2^32, so they
    stand for ``top``) on both its stems, and the crossing element
    c = cross_at[i % len]. Batch 1 takes its keys to C0 = near - 1 - s with one
    request. In batch 2 the elements before c add h = (L - C0) // (c + 1) each
    (the first one passes near), element c lands on L + 1 + s' and the elements
    after it add 0..2. Returns (batch1, batch2, hot-request mask of batch 2)."""
    ten = np.asarray(ten, np.int64)
    hot = np.asarray(hot, np.int64)
    h1 = np.ones(hot.size, np.uint32)
    h2 = np.ones(ten.size, np.uint32)
    lim2 = {}
    for i, t in enumerate(hot.tolist()):
        pos = np.nonzero(ten == t)[0]
        r = pos.size
        L = int(limits[i % len(limits)])
        L = top if L >= 2 ** 32 - 2 else L
        c = {"first": 0, "mid": r // 2, "last": r - 1}[cross_at[i % len(cross_at)]]
        c0 = near_threshold(L, ratio) - 1 - int(rng.integers(0, 4))
        h = (L - c0) // (c + 1)
        seq = [h] * c + [L + 1 + int(rng.integers(0, 4)) - (c0 + c * h)] + rng.integers(0, 3, r - c - 1).tolist()
        assert c0 >= 1 and min(seq[:c + 1]) >= 1 and c0 + sum(max(1, x) for x in seq) <= U32_MAX
        h1[i] = c0
        h2[pos] = seq
        lim2[t] = L
    b1 = W.c1_batch(hot, now, h1)
    b2 = W.c1_batch(ten, now, h2)
    b1[0]["limit"][:] = np.repeat(np.array([lim2[t] for t in hot.tolist()], np.uint32), 2)
    mask = np.isin(ten, hot)
    b2[0]["limit"][np.repeat(mask, 2)] = np.repeat(np.array([lim2[t] for t in ten[mask].tolist()], np.uint32), 2)
    return b1, b2, mask


def run_lengths(a, n):
    """Per descriptor, how many descriptors of the batch share its stem."""
    stems = stems_of(a, n)
    cnt = {}
    for s in stems:
        cnt[s] = cnt.get(s, 0) + 1
    return [cnt[s] for s in stems]


def explain(got, want, model, a, n, what=""):
    """The failure message: for the first five differing descriptors the index,
    the run length of its stem, the model's before / after and both answers."""
    lines = []
    for f in ("code", "limit_remaining", "reset_s"):
        bad = np.nonzero(np.asarray(got[f][:n]) != np.asarray(want[f][:n]))[0]
        if bad.size:
            rl = run_lengths(a, n)
            for i in bad[:5].tolist():
                lines.append("%s %s[%d]: run of %d, limit %d hits %d unit %d, model before %s after %s; got %d want %d"
                             % (what, f, i, rl[i], a["limit"][i], a["hits"][i], a["unit"][i],
                                model["before"][i] if model else "?", model["after"][i] if model else "?",
                                got[f][i], want[f][i]))
            lines.append("%s %s: %d of %d differ" % (what, f, bad.size, n))
    if not np.array_equal(got["stats"], want["stats"]):
        lines.append("%s stats: got %s want %s" % (what, got["stats"].tolist(), want["stats"].tolist()))
    return "\n".join(lines)


# --------------------------------------------------------------------------- the streams
def _epoch_back(now0, unit):
    """A clock with one more window of `unit` above it inside the epoch."""
    return now0 - DIV[unit] if now0 > 2 ** 31 else now0


def s_once(now0):
    """Path 1. ~2k distinct tenants, 3 batches in one window: every key is seen
    once per batch (arrival order), the second and third batch on a large before."""
    rng = np.random.default_rng(101)
    run = {}
    out = []
    for k in range(3):
        b = W.c1_batch(rng.permutation(2000), now0)
        scale(b[0], b[1], rng, LIMIT_EDGES, HITS_EDGES, running=run)
        out.append(b)
    return out


def mixed_hits(rng):
    """Mostly small addends (0..8), now and then one from HITS_EDGES: a run keeps
    moving after a large addend took its key near the top."""
    return int(rng.integers(0, 9)) if rng.random() < 0.7 else HITS_EDGES[rng.integers(len(HITS_EDGES))]


def small_hits(rng):
    """Addends up to 2^19: thousands of them end a run's sum just under 2^32."""
    return int(rng.integers(0, 2 ** 19 + 1))


def _epoch_back(now0, unit):
    """A clock with one more window of `unit` above it inside the epoch."""
    return now0 - DIV[unit] if now0 > 2 ** 31 else now0


def s_once(now0):
    """Path 1. 2k distinct tenants, 3 batches in one window: every key is seen
    once per batch (arrival order); the second and third see a large before.
    The last batch keeps nothing back (reserve 0): its large addends fill
    their keys to exactly 2^32 - 1, and 200 tenants new in it can take an
    addend of 2^32 - 1 whole."""
    rng = np.random.default_rng(101)
    run, out = {}, []
    for k in range(3):
        b = W.c1_batch(rng.permutation(2000 if k < 2 else 2200), now0)
        scale(b[0], b[1], rng, LIMIT_EDGES, HITS_EDGES, running=run, reserve=1024 if k < 2 else 0, p_shadow=0.15)
        out.append(b)
    return out


def _runs(seed, now0, n_hot, lo, hi, n_scaled, singles):
    """n_hot crossing runs (crossing_runs) and n_scaled runs left to scale, of
    lo..hi-1 requests each, among `singles` tenants seen once; a third batch of
    the same tenants, all scaled, continues every key."""
    rng = np.random.default_rng(seed)
    hot = np.arange(n_hot)
    ten = rng.permutation(np.r_[np.repeat(hot, rng.integers(lo, hi, n_hot)),
                                np.repeat(5000 + np.arange(n_scaled), rng.integers(lo, hi, n_scaled)),
                                100_000 + rng.permutation(1_000_000)[:singles]])
    b1, b2, mask = crossing_runs(ten, hot, now0, rng, [2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32 - 1, 2 ** 31, 2 ** 32 - 2])
    run = {}
    account(b1[0], b1[1], run)
    account(b2[0], b2[1], run, requests=mask)
    scale(b2[0], b2[1], rng, LIMIT_EDGES, mixed_hits, running=run, requests=~mask, p_shadow=0.15)
    b3 = W.c1_batch(rng.permutation(ten), now0)
    scale(b3[0], b3[1], rng, LIMIT_EDGES, mixed_hits, running=run, p_shadow=0.15)
    return [b1, b2, b3]


def s_short(now0):
    """Path 2. 200 tenants x 3..20 requests (replay_simple), 60 of them crossing
    near and the limit at their first, a middle or their last element."""
    return _runs(102, now0, 60, 3, 21, 140, 0)


def s_long(now0):
    """Path 3. 60 runs of 33..120 requests (RUN_FAST: k_fast_over / k_fast_emit)
    among 3k tenants seen once, over 256-position block boundaries; 45 of the
    runs cross near and the limit at their first, a middle or their last element."""
    return _runs(103, now0, 45, 33, 121, 15, 3000)


def s_split(now0):
    """Path 4. ~3.7k stems of Zipf tenants; run with debug_hash_bits=13 their
    sort keys collide and k_split takes the mixed runs apart."""
    rng = np.random.default_rng(104)
    z = W.ZipfSampler(4000, 1.1)
    run, out = {}, []
    for _ in range(3):
        b = W.c1_batch(z.sample(rng, 4000), now0)
        scale(b[0], b[1], rng, LIMIT_EDGES, mixed_hits, running=run, reserve=1 << 14)
        out.append(b)
    return out


def _pin(run, tenants, limits):
    """Fix the limits of the tenants' (sec, min) stems for the stream."""
    for t, (ls, lm) in zip(tenants, limits):
        run.setdefault("limit", {})[(b"bench_tenant_t%010d_tier_sec_" % t, 0)] = ls
        run["limit"][(b"bench_tenant_t%010d_tier_min_" % t, 1)] = lm


def s_split_long(now0):
    """Path 5. 3 tenants (debug_hash_bits=1: two sort keys), runs of thousands:
    batch 1 takes the hottest keys to 2^31 + 2^30, then addends up to 2^19 until
    the budget clips them to 1: the hottest run's sum ends just under 2^32."""
    rng = np.random.default_rng(105)
    z = W.ZipfSampler(3, 1.1)
    run = {}
    _pin(run, [0, 1, 2], [(2 ** 31 + 2 ** 30 + 2 ** 29, 2 ** 32 - 1), (2 ** 31 + 2 ** 30 + 2 ** 28, 2 ** 32 - 2),
                          (2 ** 31 + 2 ** 27, 2 ** 31 - 1)])
    b1 = W.c1_batch([0, 1, 2], now0)
    first = iter([2 ** 31 + 2 ** 30 - 7, 2 ** 31 + 2 ** 30, 2 ** 31 + 5])
    scale(b1[0], b1[1], rng, LIMIT_EDGES, lambda _rng: next(first), running=run)
    out = [b1]
    for _ in range(2):
        b = W.c1_batch(z.sample(rng, 4000), now0)
        scale(b[0], b[1], rng, LIMIT_EDGES, small_hits, running=run, reserve=1 << 14)
        out.append(b)
    return out


def _alias(seed, now0, rpb, batches, now_of=None):
    rng = np.random.default_rng(seed)
    z = W.ZipfSampler(2000, 1.1)
    run, out = {}, []
    for _ in range(batches):
        now = now0 if now_of is None else now_of(rpb)
        b = W.c2u_batch(z.sample(rng, rpb), now, np.ones(rpb, np.uint32), rng, 16, 0.5)
        scale(b[0], b[1], rng, LIMIT_EDGES, mixed_hits, running=run, reserve=1 << 15, p_shadow=0.15)
        out.append(b)
    return out


def s_alias(now0):
    """Path 6. Hot stems under SECOND and MINUTE (per-request overrides whose
    limit is drawn like every other): the parallel alias path."""
    return _alias(106, now0, 4000, 3)


def s_exact(now0):
    """Path 7. As path 6 with the clock moving by a second halfway through each
    batch: multi-unit stems without one `now` take general_step."""
    return _alias(107, now0, 3000, 3, lambda nq: now0 + (np.arange(nq) >= nq // 2).astype(np.int64))


BIG_HOT = 2100


def s_big(now0):
    """Path 8. One tenant with BIG_HOT requests: each of its two stems puts more
    than 2048 descriptors into one sort bucket. Its keys start at 2^31 - 2^27,
    pass 2^31 a few hundred elements into the first big run, and cross their
    limits there (sec: 2^31 + 1) and in the second one (min: 2^31 + 2^28)."""
    rng = np.random.default_rng(108)
    run = {}
    _pin(run, [7], [(2 ** 31 + 1, 2 ** 31 + 2 ** 28)])
    b1 = W.c1_batch([7], now0)
    scale(b1[0], b1[1], rng, LIMIT_EDGES, [2 ** 31 - 2 ** 27], running=run)
    out = [b1]
    for _ in range(2):
        b = W.c1_batch(rng.permutation(np.r_[np.full(BIG_HOT, 7), 100 + np.arange(1500)]), now0)
        scale(b[0], b[1], rng, LIMIT_EDGES, small_hits, running=run, reserve=1 << 14)
        out.append(b)
    return out


def _history(seed, now0, unit):
    rng = np.random.default_rng(seed)
    t0, d = _epoch_back(now0, unit), DIV[unit]
    run, out = {}, []
    for k, now in enumerate((t0, t0 + d, t0, t0 + d)):
        ten = rng.permutation(np.r_[np.arange(300), np.full(60 if k >= 2 else 1, 999)])
        b = W.c1_batch(ten, now)
        b[0]["unit"][:] = unit
        scale(b[0], b[1], rng, LIMIT_EDGES, mixed_hits if k >= 2 else HITS_EDGES, running=run)
        out.append(b)
    return out


def s_history_second(now0):
    """Path 9, SECOND. Keys counted to above 2^31 in window w, moved to w + 1,
    then requests back in w (the count comes back from the history log), one
    tenant as a run of 60 on the older window; then w + 1 again."""
    return _history(109, now0, 1)


def s_history_minute(now0):
    """Path 9, MINUTE."""
    return _history(110, now0, 2)


def s_zero_units(_now0=None):
    """Clock 0 and 59 with HOUR and DAY descriptors: windowStart 0, reset
    3600 - now and 86400 - now."""
    rng = np.random.default_rng(111)
    run, out = {}, []
    for now in (0, 0, 59):
        b = W.c1_batch(rng.permutation(500), now)
        b[0]["unit"][:] = np.tile(np.array([3, 4], np.uint8), 500)
        scale(b[0], b[1], rng, LIMIT_EDGES, HITS_EDGES, running=run)
        out.append(b)
    return out


TOP_BAD = 250  # the request of s_top's second batch whose clock is NOW_MAX + 1


def s_top(_now0=None):
    """The top of the clock range: a batch at NOW_MAX - 2 (SECOND and DAY), one at
    exactly NOW_MAX (DAY) with request TOP_BAD at NOW_MAX + 1 in the middle of it
    (RL_E_TIME, alone), and after rl_sweep(NOW_MAX) one more at NOW_MAX."""
    rng = np.random.default_rng(112)
    run, out = {}, []
    for k, now in enumerate((NOW_MAX - 2, NOW_MAX, NOW_MAX)):
        b = W.c1_batch(rng.permutation(500), now)
        b[0]["unit"][:] = np.tile(np.array([4, 4] if k == 1 else [1, 4], np.uint8), 500)
        scale(b[0], b[1], rng, LIMIT_EDGES, HITS_EDGES, running=run)
        out.append(b)
    out[1][0]["now"][TOP_BAD] = NOW_MAX + 1
    return out


def top_keep(b):
    """The descriptors of s_top's second batch that are answered."""
    return b[0]["req_idx"][:b[1]] != TOP_BAD


def s_counted(now0):
    """Three tenants counted to 2^31 - 1, 2^31 and 2^32 - 1 by one request each
    (the last one over its limit: a local-cache entry where that is on)."""
    a, n, nq, nr = W.c1_batch([0, 1, 2], now0, [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1])
    a["limit"][:] = np.repeat(np.array([2 ** 31, 2 ** 31, 2 ** 32 - 2], np.uint32), 2)
    return [(a, n, nq, nr)]


STREAMS = {"once": s_once, "short": s_short, "long": s_long, "split": s_split, "split_long": s_split_long,
           "alias": s_alias, "exact": s_exact, "big": s_big, "history_second": s_history_second,
           "history_minute": s_history_minute, "zero_units": s_zero_units, "top": s_top, "counted": s_counted}
EPOCH_FREE = ("zero_units", "top")  # (their clocks are their own)


@functools.lru_cache(maxsize=None)
def stream(name, epoch="now0"):
    """The stream `name` at a clock epoch: built once, shared by every test (and
    by the CPU and GPU files), never modified."""
    return STREAMS[name](CLOCK_EPOCHS[epoch])


def oracle_input(name, batches):
    """What the oracles are fed: the stream itself, except that `top` goes
    without the request the engine must refuse."""
    if name != "top":
        return batches
    import streams
    a, n, nq, nr = batches[1]
    d, dn, dq = streams.drop_descriptors(a, n, nq, top_keep(batches[1]))
    d["now"] = np.minimum(d["now"], NOW_MAX)  # (the dropped request keeps its slot; it has no descriptor)
    return [batches[0], (d, dn, dq, nr), batches[2]]


@functools.lru_cache(maxsize=None)
def reference(name, epoch, lc, ratio=0.8):
    """(C oracle results, model results or None) for a stream, computed once."""
    from oracle import c_oracle
    bs = oracle_input(name, stream(name, epoch))
    co = c_oracle.COracle(ratio, lc)
    want = [co.do_limit(*b) for b in bs]
    co.close()
    return want, exact_model(bs, ratio, lc)


def coverage(name, bs, model, lc):
    """What every path stream must hold: OK and OVER_LIMIT answers, a before
    above 2^31, and with the local cache on at least one hit of it."""
    codes = np.concatenate([m["code"] for m in model])
    assert (codes == OK).any() and (codes == OVER).any(), name
    assert max(b for m in model for b in m["before"] if b is not None) > 2 ** 31, name
    if lc:
        assert sum(int(m["lc_hit"].sum()) for m in model) > 0, name


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def golden_batches(cases, lc):
    """Step k of every known-answer case (of that local-cache setting) as batch
    k: one stem per case, one descriptor per request."""
    cs = [c for c in cases if bool(c.get("local_cache")) == lc]
    from ratelimit_amd.packing import arrays_from_lists
    out = []
    for k in range(max(len(c["hits"]) for c in cs)):
        live = [(j, c) for j, c in enumerate(cs) if k < len(c["hits"])]
        n = len(live)
        a = arrays_from_lists([b"edge_case_%d_" % j for j, _ in live], [c["now"] for _, c in live], list(range(n)),
                              [c["unit"] for _, c in live], [1 if c.get("shadow") else 0 for _, c in live],
                              [c["limit"] for _, c in live], [c["hits"][k] for _, c in live], [0] * n)
        out.append(((a, n, n, 1), [tuple(c["expect"][k]) for _, c in live], [c["name"] for _, c in live]))
    return out


# --------------------------------------------------------------------------- the decide grid
BEFORE_EDGES = sorted(set(LIMIT_EDGES + HITS_EDGES))


@functools.lru_cache(maxsize=None)
def decide_grid():
    """(before, after, lc_hit, hits, limit, shadow) over before x hits x limit
    with before + max(1, hits) <= 2^32 - 1, shadow and local-cache hit on and off.
    `hits` is what GetResponseDescriptorStatus is handed: max(1, hits_addend)."""
    out = []
    for before in BEFORE_EDGES:
        for h in sorted({max(1, x) for x in HITS_EDGES}):
            if before + h > U32_MAX:
                continue
            for limit in LIMIT_EDGES:
                for shadow in (False, True):
                    for lc_hit in (False, True):
                        out.append((before, before + h, lc_hit, h, limit, shadow))
    return out


def python_decide(ratio, lc_enabled, case):
    """The Python oracle's GetResponseDescriptorStatus on one grid case ->
    (code, remaining, stat deltas, local cache set)."""
    before, after, lc_hit, h, limit, shadow = case
    oc = O.OracleFixedRateLimitCache(ratio, lc_enabled)
    rl = O.RateLimit("r", O.RateLimitStats("r"), O.Limit(limit, O.MINUTE), False, shadow)
    st = oc.get_response_descriptor_status("k", rl, before, after, lc_hit, h, 0)
    return st.code, st.limit_remaining, rl.stats.as_tuple(), bool(lc_enabled and oc.local_cache.data)


def primed_stream(seed, limit_range, prime, start_now=1_700_000_035, **kw):
    """streams.random_stream with limits drawn from limit_range, behind one
    priming call per (domain, entries, unit) of the stream that takes its key
    of the first window to `prime`. The stream's own addends are small
    (kw max_hits), so counts walk across the limits one to three at a time."""
    import streams
    calls = streams.random_stream(seed, limit_range=limit_range, start_now=start_now, **kw)
    seen = {}
    for req, limits, _ in calls:
        for d, l in zip(req.descriptors, limits):
            if l is not None:
                seen.setdefault((req.domain, tuple(d.entries), l.limit.unit), (d, l))
    return [(O.RateLimitRequest(dom, [d], prime), [l], start_now) for (dom, _, _), (d, l) in seen.items()] + calls


RANDOM_KW = dict(n_stems=3, max_step=1, max_hits=3, max_desc=2, p_nil=0.0, domains=("dom",))
RANDOM_MAX_ADDEND, RANDOM_MAX_DESC = 3, 2  # (random_stream's own addends are 0..3 at max_hits=3)


def random_worst(n_calls):
    """What one key can take after its priming: every descriptor of every call, the largest addend."""
    return n_calls * RANDOM_MAX_DESC * RANDOM_MAX_ADDEND


# where -> (n_calls, limit_range, priming count). A key typically takes a fifth of the worst
# case, so the limits lie within that reach of the priming count, and the worst case still
# ends at or below 2^32 - 1: 24 calls -> 144, primed to 2^32 - 145, limits 2^32 - 128 +- 16.
RANDOM_RANGES = {"sign": (40, (2 ** 31 - 64, 2 ** 31 + 64), 2 ** 31 - 30),
                 "top": (24, (2 ** 32 - 144, 2 ** 32 - 112), 2 ** 32 - 1 - random_worst(24))}
# (top, seed 4: no key reaches its limit within the 24 calls, every answer is OK)
RANDOM_CASES = [(w, s) for w in sorted(RANDOM_RANGES) for s in range(7) if (w, s) != ("top", 4)]
