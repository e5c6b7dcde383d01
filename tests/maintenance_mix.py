"""The maintenance calls in combination: what tests/test_maintenance_mix_cpu.py
and tests/test_gpu_maintenance_mix.py share. Host code only: the plan (one
request stream, ten maintenance operations ordered so that every ordered pair
of them occurs back to back), the oracle side of every operation, and the
checkers that compare every reader of the table with the Python oracle.

The stream is test_gpu_forget.fg_stream's (its rule registry, domains, entry
shapes and Zipf weights) at 400 stems, with two additions: late calls, whose
clock runs 1..7 s (SECOND stems) or 1..3 windows (MINUTE stems) behind the
running clock, so that history chains are read and not only written; and clock
jumps, so that a walk of a few thousand calls spans more than the sweep's lag.

A Walk is one quarter of the schedule with its own oracle and stream. It is
driven step by step by the CPU test (the oracle alone, and a fake reader built
from the oracle) and by the GPU test (a cache, read through GpuReader); both
make the same calls in the same order, so what the CPU test proves about the
plan holds for the GPU run.
"""
import random

import scan_cases as SC
from oracle import oracle as O
from ratelimit_amd import abi
from ratelimit_amd.packing import stem_of
import streams
from test_gpu_forget import DIV, NEVER, arena_bytes, oracle_forget, st, stats_of

OPS = ("F_KEYS", "F_PREFIX", "SWEEP", "T_SMALL", "T_LARGE", "H_SMALL", "H_LARGE", "ARENA", "SNAPSHOT", "MIGRATE")
PRESERVING = OPS[3:]            # the oracle side of these is: nothing
LAG = 600                       # the sweep's floor runs this far behind the clock: above the furthest late call (180 s)
SLOTS = (1 << 10, 1 << 13)      # T_SMALL, T_LARGE
# The history log's floor: at 2^19 a partition holds 8192 entries, and a walk's
# appends, summed over the ctxs it uses, must stay below a partition's size so
# that no partition can wrap or refuse. The CPU count (Walk.appends, checked by
# test_the_plan_stays_in_range) is an upper estimate: one append per write into
# another window than the key's newest, every older record once more per
# MIGRATE, and the entries of every image a SNAPSHOT loads, which count as the
# new ctx's appends. It gives 4900 to 7100 a walk; the GPU walks measure 2600
# to 4000.
H_FLOOR = 1 << 19
ARENAS = (1 << 17, 1 << 19)     # both far above a walk's long-stem bytes (below 10 000)
SEG_CALLS, PRELUDE_CALLS, N_STEMS = 120, 720, 400
START = 1_700_000_030
# walk: (local cache, per_second, shards at start, debug_hash_bits, cache key prefix)
WALKS = ((True, False, 1, 0, ""), (False, True, 2, 0, ""), (True, True, 1, 5, ""), (False, False, 2, 0, "mix:"))
CTX = dict(table_slots=1 << 13, max_batch=1 << 12, max_rules=1 << 10, hash_seed=17, history_entries=H_FLOOR,
           arena_bytes=ARENAS[0])


# --------------------------------------------------------------------------- the schedule
def euler_circuit(seed=4):
    """The ops as a closed walk over every edge of the complete directed graph on
    them, self-loops included: 101 vertices, the last equal to the first, each
    ordered pair once among the 100 consecutive pairs (Hierholzer)."""
    rng = random.Random(seed)
    out_edges = {a: list(OPS) for a in OPS}
    for a in OPS:
        rng.shuffle(out_edges[a])
    stack, circuit = [OPS[0]], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def pair_table():
    """The schedule as a matrix: row = a call, column = the call that follows it
    after one segment, cell = walk.step of the second call."""
    at = {}
    for k in range(4):
        ops = walk_ops(k)
        for i in range(1, len(ops)):
            at[(ops[i - 1], ops[i])] = "%d.%d" % (k, i)
    rows = ["%-9s" % "" + " ".join("%-8s" % b for b in OPS)]
    rows += ["%-9s" % a + " ".join("%-8s" % at[(a, b)] for b in OPS) for a in OPS]
    return "\n".join(r.rstrip() for r in rows)


def walk_ops(k):
    """Walk k's 26 ops: the circuit's steps 25 k .. 25 k + 24, after its
    predecessor's last op as step 0, so that no pair falls into a cut."""
    c = euler_circuit()[:100]
    return [c[(25 * k - 1) % 100]] + c[25 * k:25 * k + 25]


# --------------------------------------------------------------------------- the stream
def mix_stream(seed, n_segments, late=0.15):
    """-> [segment][(request, limits, now)], segment 0 the prelude. fg_stream's
    iteration (1..3 descriptors at the running clock, a request per domain), or
    with probability `late` one descriptor of a SECOND / MINUTE stem at an
    earlier clock (and four such calls begin every segment but the prelude).
    The clock also jumps 60 s after every 60 calls of the prelude and 40 s in
    the middle of every other segment."""
    rng = random.Random(seed)
    reg = {}

    def rule(s, unit):
        if (s % 7, unit) not in reg:
            reg[(s % 7, unit)] = O.new_rate_limit(5 + 3 * (s % 7), unit, "fg_rule%d_u%d" % (s % 7, unit),
                                                  shadow_mode=(s % 11 == 0 and unit != O.HOUR))
        return reg[(s % 7, unit)]

    def entries(s):
        e = [("stem", "s%03d" % s)]
        if s % 5 == 2:
            e.append(("path", "/a/rather/long/path/component/%03d" % s))
        return e

    w = [1.0 / (i + 1) ** 1.1 for i in range(N_STEMS)]
    units = [(O.SECOND, O.MINUTE, O.MINUTE, O.SECOND, O.DAY, O.MINUTE)[s % 6] for s in range(N_STEMS)]
    segments, now = [], START
    for seg in range(n_segments):
        calls, size, jumped = [], PRELUDE_CALLS if seg == 0 else SEG_CALLS, 0
        while len(calls) < size:
            if (seg and len(calls) < 4) or (calls and rng.random() < late):  # (the clock stands at the last call's)
                # a segment after a step begins with four late calls of the busiest SECOND / MINUTE stems
                s = rng.choice((0, 1, 2, 3, 5)) if seg and len(calls) < 4 else rng.choices(range(N_STEMS), w)[0]
                back = {O.SECOND: rng.randint(1, 7), O.MINUTE: 60 * rng.randint(1, 3)}.get(units[s], 0)
                calls.append((O.RateLimitRequest("fg" if s % 3 else "fg_b", [O.Descriptor(entries(s))],
                                                 rng.randint(1, 4)), [rule(s, units[s])], max(now - back, START)))
                continue
            now += rng.choice([0] * 60 + [1, 1, 1, 2, 20])
            if seg == 0 and len(calls) // 60 > jumped:
                now, jumped = now + 60, len(calls) // 60
            elif seg and not jumped and len(calls) >= size // 2:
                now, jumped = now + 40, 1
            per_dom = {}
            for _d in range(rng.randint(1, 3)):
                s = rng.choices(range(N_STEMS), w)[0]
                unit = O.HOUR if s % 6 == 1 and rng.random() < 0.3 else units[s]
                d, l = per_dom.setdefault("fg" if s % 3 else "fg_b", ([], []))
                d.append(O.Descriptor(entries(s)))
                l.append(rule(s, unit))
            for dom, (d, l) in per_dom.items():
                calls.append((O.RateLimitRequest(dom, d, rng.randint(1, 4)), l, now))
        segments.append(calls)
    return segments


def clone(oc):
    """A copy of the oracle's stores (rules and their stats are the stream's)."""
    c = O.OracleFixedRateLimitCache(0.8, oc.local_cache is not None, oc.prefix, oc.per_second_client is not None)
    c.client.data = {k: list(e) for k, e in oc.client.data.items()}
    if oc.per_second_client is not None:
        c.per_second_client.data = {k: list(e) for k, e in oc.per_second_client.data.items()}
    if oc.local_cache is not None:
        c.local_cache.data = dict(oc.local_cache.data)
    return c


# --------------------------------------------------------------------------- a walk
class Walk:
    """One walk's plan and oracle. The driver alternates segment(i) and, for
    step i, args(i) -> the GPU call -> apply(i, a); `model` holds the windows
    written per (stem, unit) since the key's last deletion or eviction, which the
    plan (not the GPU checks) is derived from."""

    def __init__(self, k):
        self.k = k
        self.lc, self.per_second, self.shards, self.hash_bits, self.prefix = WALKS[k]
        self.ops = walk_ops(k)
        self.segments = mix_stream(100 + k, len(self.ops) + 1)
        self.oc = O.OracleFixedRateLimitCache(0.8, self.lc, self.prefix, self.per_second)
        self.model = {}          # (stem, unit) -> {ws: the tick of its last write}
        self.tick = 0            # calls made so far
        self.step_tick = 0       # ... at the last step
        self.now = START
        self.floor = 0
        self.slots, self.history, self.arena, self.seed = CTX["table_slots"], H_FLOOR, ARENAS[0], CTX["hash_seed"]
        self.forgotten = set()   # stems deleted and not hit since
        self.deleted = []        # (stem, unit, ws) of deleted windows, the newest last
        self.tomb_zero = True    # no tombstone can exist: set by a resize or a migrate, cleared by a deletion
        self.late_reads = 0      # late calls that read a window written before the last step
        self.appends = [0]       # per ctx: an upper estimate of history_appended
        self.written = 0         # entries the current log holds (a loaded image brings them along)
        self.answers, self.snaps, self.applied = [], [], []

    # ---- the stream
    def store(self, unit):
        return self.oc.per_second_client if self.per_second and unit == O.SECOND else self.oc.client

    def segment(self, i):
        """The oracle over segment i -> ([[status tuple]] per call, the per-rule stats
        deltas). Updates the model."""
        out = []
        streams.reset_stats(self.segments[i])
        for r, lims, now in self.segments[i]:
            late = now < self.now
            self.now = max(self.now, now)
            for d, lim in zip(r.descriptors, lims):
                u = lim.limit.unit
                stem, ws = stem_of(self.prefix, r.domain, d.entries), now // DIV[u] * DIV[u]
                self.forgotten.discard(stem)
                if self.lc and self.oc.local_cache.data.get(stem.decode() + str(ws), 0) > now:
                    continue  # answered by the local cache: nothing is written
                wins = self.model.setdefault((stem, u), {})
                if late and wins.get(ws, self.tick) < self.step_tick:
                    self.late_reads += 1
                if wins and ws != max(wins):  # the newest window moves, or an older one gets another version
                    self.appends[-1] += 1
                    self.written += 1
                wins[ws] = self.tick
            out.append([st(s) for s in self.oc.do_limit(r, lims, now)])
            self.tick += 1
        self.answers.append((out, stats_of(self.segments[i])))
        return self.answers[-1]

    def key_records(self, key, oc=None):
        """[(ws, count, expire, lc)] of a model key as the oracle holds them, oldest first."""
        oc = oc or self.oc
        stem, unit = key
        store = oc.per_second_client if self.per_second and unit == O.SECOND else oc.client
        out = []
        for ws in sorted(self.model[key]):
            e = store.data.get(stem.decode() + str(ws))
            if e is not None:
                out.append((ws, e[0], e[1], oc.local_cache.data.get(stem.decode() + str(ws), 0) if self.lc else 0))
        return out

    def evictable(self, floor):
        """The model keys whose every record and local-cache entry has expired at floor."""
        return [k for k in self.model if all(floor > e and lc <= floor for _, _, e, lc in self.key_records(k))]

    # ---- the plan of one step
    def _future(self, i):
        """{stem: calls until it is hit again, (stem, unit): ... under that unit} over the segments after step i."""
        seen, n = {}, 0
        for seg in self.segments[i + 1:]:
            for r, lims, _ in seg:
                for d, lim in zip(r.descriptors, lims):
                    stem = stem_of(self.prefix, r.domain, d.entries)
                    seen.setdefault(stem, n)
                    seen.setdefault((stem, lim.limit.unit), n)
                n += 1
        return seen

    def args(self, i):
        """What step i's call is given, from the oracle side alone."""
        op = self.ops[i]
        if op == "F_KEYS":
            fut = self._future(i)
            stems = sorted({k[0] for k in self.model if k[0] in fut}, key=lambda s: (fut[s], s))
            live = lambda s, u: any(e >= self.now for _, _, e, _ in self.key_records((s, u)))
            soon = lambda u: sorted((s for s in stems if (s, u) in fut), key=lambda s: (fut[(s, u)], s))
            kinds = {
                "two_units": [s for s in soon(O.HOUR) if (s, O.MINUTE) in self.model and (s, O.HOUR) in self.model and
                              live(s, O.HOUR)],
                "day": [s for s in soon(O.DAY) if (s, O.DAY) in self.model],
                "long": [s for s in stems if len(s) > 36],
                "history": [s for s in stems if any(k[0] == s and len(w) >= 2 for k, w in self.model.items())],
                "blocked": [s for s in stems if self.lc and any(
                    k.rstrip("0123456789") == s.decode() and e > self.now for k, e in self.oc.local_cache.data.items())],
            }
            chosen = []
            for kind, lst in kinds.items():
                if kind == "blocked" and not self.lc:
                    continue
                assert lst, (self.k, i, kind)
                chosen += [s for s in lst[:2] if s not in chosen]
            return chosen + [self.prefix.encode() + NEVER]
        if op == "F_PREFIX":
            fut = self._future(i)
            longs = sorted((s for s, _ in self.model if len(s) > 36 and s in fut), key=lambda s: (fut[s], s))
            assert longs, (self.k, i)
            # one domain's stems s000 .. s099 (a few dozen keys, the busiest among them), and a prefix that ends
            # inside a long stem's arena part
            return [self.prefix.encode() + (b"fg_stem_s0", b"fg_b_stem_s0")[i % 2], longs[0][:len(longs[0]) - 9]]
        if op == "SWEEP":
            return self.now - LAG
        if op in ("T_SMALL", "T_LARGE"):
            return SLOTS[op == "T_LARGE"]
        if op in ("H_SMALL", "H_LARGE"):
            return H_FLOOR * (4 if op == "H_LARGE" else 1)
        if op == "ARENA":
            return ARENAS[self.arena == ARENAS[0]]
        if op == "MIGRATE":
            return dict(hash_seed=self.seed + 1, n_shards=3 - self.shards, table_slots=SLOTS[self.slots == SLOTS[0]])
        return None

    def apply(self, i, a):
        """The oracle side of step i (and the plan's bookkeeping). -> oracle keys deleted."""
        op, n = self.ops[i], 0
        self.snaps.append((clone(self.oc), {k: dict(w) for k, w in self.model.items()}))
        self.applied.append((op, a))
        self.step_tick = self.tick
        if op in ("F_KEYS", "F_PREFIX"):
            gone = [k for k in self.model if (k[0] in a if op == "F_KEYS" else any(k[0].startswith(p) for p in a))]
            for k in gone:
                self.deleted += [(k[0], k[1], ws) for ws in sorted(self.model[k])]
                self.forgotten.add(k[0])
                del self.model[k]
            n = oracle_forget(self.oc, **{"stems" if op == "F_KEYS" else "prefixes": a})
            self.tomb_zero = self.tomb_zero and not gone
        elif op == "SWEEP":
            gone = self.evictable(a)
            for k in gone:
                del self.model[k]
            self.floor, n = max(self.floor, a), len(gone)
            self.tomb_zero = self.tomb_zero and not gone
        elif op in ("T_SMALL", "T_LARGE"):
            self.slots, self.tomb_zero = a, True
        elif op in ("H_SMALL", "H_LARGE"):
            self.history = a
            self.written = sum(len(w) - 1 for w in self.model.values())  # the garbage is gone
        elif op == "ARENA":
            self.arena = a
        elif op == "SNAPSHOT":
            self.appends.append(self.written)  # the image's entries count as the new ctx's appends
        elif op == "MIGRATE":
            self.seed, self.shards, self.slots, self.tomb_zero = a["hash_seed"], a["n_shards"], a["table_slots"], True
            self.written = sum(len(w) - 1 for w in self.model.values())  # every older record is appended again
            self.appends.append(self.written)
        return n

    def replay(self, oc, i, until=None):
        """Another oracle from step i on (the caller has made its version of step
        i): the later steps' deletions applied as they were, segment by segment.
        -> the first segment index at which an answer or a stats delta differs
        from the walk's own, or None; stops before step `until`."""
        for j in range(i, len(self.ops)):
            if until is not None and j >= until:
                return None
            op, a = self.applied[j]
            if op in ("F_KEYS", "F_PREFIX") and j != i:
                oracle_forget(oc, **{"stems" if op == "F_KEYS" else "prefixes": a})
            streams.reset_stats(self.segments[j + 1])
            got = [[st(s) for s in oc.do_limit(r, lims, now)] for r, lims, now in self.segments[j + 1]]
            if (got, stats_of(self.segments[j + 1])) != self.answers[j + 1]:
                return j + 1
        return None


def without_older_windows(wk, oc, model):
    """Delete from oc every window of every model key but the key's newest (and
    what another unit of the stem holds as its newest). -> keys deleted."""
    keep = {(k[0], max(w)) for k, w in model.items()}
    n = 0
    for (stem, unit), wins in model.items():
        store = oc.per_second_client if wk.per_second and unit == O.SECOND else oc.client
        for ws in wins:
            if (stem, ws) not in keep and store.data.pop(stem.decode() + str(ws), None) is not None:
                n += 1
                if wk.lc:
                    oc.local_cache.data.pop(stem.decode() + str(ws), None)
    return n


# --------------------------------------------------------------------------- the readers
class _FloorTap:
    """Backend.scan, noting every page's time_floor (scan_cases.scan_all sums the other fields)."""

    def __init__(self, be):
        self.be, self.floors = be, set()

    def scan(self, **kw):
        for rec, d, b in self.be.scan(**kw):
            self.floors.add(d["time_floor"])
            yield rec, d, b


class GpuReader:
    """The table's readers as the checkers call them."""

    def __init__(self, be):
        self.be = be

    def export(self):
        return SC.export_list(self.be)

    def scan(self, **kw):
        tap = _FloorTap(self.be)
        recs, info, byp, pages = SC.scan_all(tap, **kw)
        return recs, info, byp, pages, tap.floors

    def hot(self, now, k, blocked):
        rec, info = self.be.hot_keys(now, k, blocked=blocked)
        assert not rec["flags"].any()
        return [(s, u, ws, c, e, lc) for s, u, f, ws, c, e, lc in SC.rec_list(rec)], info

    def lookup(self, stems, units, nows):
        return {k: v.tolist() for k, v in self.be.lookup(stems, units, nows).items()}

    def table_info(self):
        return self.be.table_info()

    def lc_entries(self, now):
        return self.be.local_cache_info(now)["entry_count"]


class FakeReader:
    """The same readers answered from the walk's oracle and model, with one
    defect at a time: what the CPU test feeds the checkers to show that each of
    them can fail. defect: None, "forgotten_kept", "older_dropped",
    "scan_older_dropped", "floor_zero", "count_off", "lookup_off", "hot_off"."""

    def __init__(self, wk, defect=None):
        self.wk, self.defect = wk, defect

    def export(self):
        wk, out = self.wk, []
        for key in sorted(wk.model):
            out += [(key[0], key[1], 0) + r for r in wk.key_records(key)]
        if self.defect == "forgotten_kept":
            s, u, ws = wk.deleted[-1]
            out.append((s, u, 0, ws, 1, ws + DIV[u], 0))
        if self.defect == "older_dropped":
            out.remove(self._live_older(out))
        if self.defect == "count_off":
            j = next(j for j, r in enumerate(out) if r[5] >= wk.now)
            out[j] = out[j][:4] + (out[j][4] + 1,) + out[j][5:]
        return out

    def _live_older(self, recs):
        return next(r for r, nxt in zip(recs, recs[1:]) if r[:2] == nxt[:2] and r[5] >= self.wk.now)

    def scan(self, **kw):
        wk = self.wk
        export = FakeReader(wk).export()
        recs, info, byp = SC.expected(export, **{k: v for k, v in kw.items() if k != "page_records"})
        if self.defect == "scan_older_dropped" and not kw.get("newest") and not kw.get("prefixes"):
            recs.remove(self._live_older(recs))
        info["slots_scanned"] = wk.shards * wk.slots
        return recs, info, byp, wk.shards, {0 if self.defect == "floor_zero" else wk.floor}

    def hot(self, now, k, blocked):
        wk = self.wk
        m = hot_matching(FakeReader(wk).export(), now, blocked)
        n = min(k, len(m))
        thr = m[n - 1][3] if n else 0
        info = {"slots": wk.shards * wk.slots, "matched": len(m), "hits": sum(r[3] for r in m),
                "above": sum(r[3] > thr for r in m[:n]), "threshold": thr, "time_floor": wk.floor}
        got = m[:n]
        if self.defect == "hot_off":
            got[0] = got[0][:3] + (got[0][3] + 1,) + got[0][4:]
        return got, info

    def lookup(self, stems, units, nows):
        wk = self.wk
        out = {k: [] for k in ("status", "found", "count", "expire", "lc")}
        for stem, unit, now in zip(stems, units, nows):
            key = stem.decode() + str(now // DIV[unit] * DIV[unit])
            e = wk.store(unit).data.get(key)
            live = e is not None and now <= e[1]
            lc = wk.oc.local_cache.data.get(key, 0) if wk.lc else 0
            for k, v in zip(out, (0, int(live), e[0] if live else 0, e[1] if live else 0, lc if lc > now else 0)):
                out[k].append(v)
        if self.defect == "lookup_off":
            j = out["found"].index(1)
            out["count"][j] += 1
        return out

    def table_info(self):
        wk = self.wk
        live = [k for k in wk.model if wk.key_records(k)]
        return {"table_slots": wk.shards * wk.slots, "live_slots": len(live), "tombstones": 0,
                "arena_bytes_used": sum(arena_bytes(k[0]) for k in live), "history_entries": wk.shards * wk.history,
                "history_lost": 0, "history_refused": 0}

    def lc_entries(self, now):
        return self.wk.oc.local_cache.entry_count(now)


# --------------------------------------------------------------------------- the checkers
def key_counts(recs):
    out = {}
    for r in recs:
        out[r] = out.get(r, 0) + 1
    return out


def live_bytes(export):
    """The arena bytes of the export's long stems, one allocation per (stem, unit)."""
    return sum(arena_bytes(g[0][0]) for g in SC.groups_of(export))


def check_export(export, wk):
    """The export against the oracle's stores at the walk's clock: the live
    (stem ‖ decimal(ws), count) pairs are the stores' live keys
    (test_gpu_scan_live_keys_are_the_oracles' rule: the first record in unit
    order stands for a Redis key that unit slots share), no chain is lost, and
    no record belongs to a stem forgotten since its last hit."""
    SC.groups_of(export)
    assert not any(r[2] & abi.RL_REC_CHAIN_LOST for r in export), "chains_lost != 0"
    kept = sorted({r[0] for r in export} & wk.forgotten)
    assert not kept, ("records of forgotten stems", kept[:3])

    def store_of(unit):
        return 1 if wk.per_second and unit == 1 else 0

    got = {}
    for r in sorted((r for r in export if wk.now <= r[5]), key=lambda r: r[1]):
        got.setdefault((store_of(r[1]), r[0].decode() + str(r[3])), (r[4], r[5]))
    stores = [wk.oc.client.data, wk.oc.per_second_client.data if wk.per_second else {}]
    want = {(i, k): (e[0], e[1]) for i, s in enumerate(stores) for k, e in s.items() if wk.now <= e[1]}
    if got != want:
        diff = sorted(set(got.items()) ^ set(want.items()))
        raise AssertionError("live records differ from the oracle's stores: %d, first %r (got %r, want %r)" % (
            len(diff), diff[0][0], got.get(diff[0][0]), want.get(diff[0][0])))
    return len(want)


def check_scans(rd, export, wk):
    """rl_scan paged a tile at a time, with NEWEST | LIVE, and under one domain
    prefix: each the filter of the export (scan_cases.expected); every page's
    time_floor is the last sweep's floor."""
    dom = [(wk.prefix + "fg_stem_").encode()]
    for kw in (dict(page_records=1), dict(newest=True, now=wk.now), dict(prefixes=dom)):
        q = {k: v for k, v in kw.items() if k != "page_records"}
        want, winfo, wbyp = SC.expected(export, **q)
        got, ginfo, gbyp, pages, floors = rd.scan(**kw)
        SC.groups_of(got)
        assert key_counts(got) == key_counts(want), ("scan", kw, len(got), len(want))
        for f, v in winfo.items():
            assert ginfo[f] == v, ("scan", f, kw, ginfo[f], v)
        assert gbyp == wbyp, ("scan by_prefix", kw)
        assert ginfo["slots_scanned"] == wk.shards * wk.slots and pages >= wk.shards, ("scan", kw, pages)
        assert floors == {wk.floor}, ("scan time_floor", kw, floors, wk.floor)
        assert want or kw.get("newest"), kw  # (the whole table and the domain are never empty)


def hot_matching(export, now, blocked):
    """rl_hot_keys' matching records in the answer's order (the header's rule), from the export."""
    newest = [g[-1] for g in SC.groups_of(export)]
    m = [(s, u, ws, c, e, lc) for s, u, f, ws, c, e, lc in newest
         if ws == now - now % DIV[u] and now <= e and (not blocked or now < lc)]
    return sorted(m, key=lambda r: (-r[3], r[0], r[1]))


def check_hot(rd, export, wk, blocked=False, k=32):
    m = hot_matching(export, wk.now, blocked)
    got, info = rd.hot(wk.now, k, blocked)
    n = min(k, len(m))
    what = ("hot_keys", wk.now, blocked)
    assert len(got) == n, what + (len(got), n)
    assert [r[3] for r in got] == [r[3] for r in m[:n]], what
    assert len(set(got)) == n and set(got) <= set(m), what
    thr = m[n - 1][3] if n else 0
    above = [r for r in m[:n] if r[3] > thr]
    assert set(above) <= set(got) and got == sorted(got, key=lambda r: (-r[3], r[0], r[1])), what
    assert info == {"slots": wk.shards * wk.slots, "matched": len(m), "hits": sum(r[3] for r in m),
                    "above": len(above), "threshold": thr, "time_floor": wk.floor}, what + (info,)
    return len(m)


def lookup_probes(wk, n=20):
    """About 3 n (stem, unit, clock): keys at the walk's clock; older windows the
    oracle still holds, read at their last second; windows of forgotten stems;
    the stem never seen. Every clock is at or above the floor and within 7
    windows of the walk's clock (where the history is exact by construction)."""
    rng = random.Random(wk.tick)
    keys = sorted(wk.model)
    probes = [(s, u, wk.now) for s, u in rng.sample(keys, min(n, len(keys)))]

    def near(u, ws):
        return ws + DIV[u] - 1 >= wk.floor and 0 <= wk.now // DIV[u] - ws // DIV[u] <= 7

    older = [(k[0], k[1], ws + DIV[k[1]] - 1) for k in keys for ws in sorted(wk.model[k])[:-1] if near(k[1], ws)]
    probes += rng.sample(older, min(n, len(older)))
    gone = [(s, u, ws + DIV[u] - 1) for s, u, ws in wk.deleted[::-1] if near(u, ws)]
    probes += gone[:n]
    probes += [(s, u, wk.now) for s, u, _ in wk.deleted[-n // 2:]]
    probes.append((wk.prefix.encode() + NEVER, 2, wk.now))
    return probes


def check_lookup(rd, wk):
    """rl_lookup against the oracle's stores, as test_gpu_lookup_reads_the_oracles_stores reads them."""
    probes = lookup_probes(wk)
    res = rd.lookup([p[0] for p in probes], [p[1] for p in probes], [p[2] for p in probes])
    assert not any(res["status"]), ("lookup status", sorted(set(res["status"])))
    n_found = 0
    for j, (stem, unit, now) in enumerate(probes):
        key = stem.decode() + str(now // DIV[unit] * DIV[unit])
        e = wk.store(unit).data.get(key)  # (read without mutation)
        live = e is not None and now <= e[1]
        got = (res["found"][j], res["count"][j], res["expire"][j])
        assert got == ((1, e[0], e[1]) if live else (0, 0, 0)), ("lookup", key, unit, now, got, e)
        lc = wk.oc.local_cache.data.get(key, 0) if wk.lc else 0
        assert res["lc"][j] == (lc if lc > now else 0), ("lookup lc", key, now)
        n_found += live
    return len(probes), n_found


def check_table_info(info, export, wk, exact_arena=None):
    """exact_arena: None where only the lower bound holds, else the exact
    arena_bytes_used ("live": the live long stems' bytes, after a sweep's compaction)."""
    if exact_arena == "live":
        exact_arena = live_bytes(export)
    assert info["live_slots"] == len(SC.groups_of(export)), ("live_slots", info["live_slots"])
    assert not wk.tomb_zero or info["tombstones"] == 0, ("tombstones", info["tombstones"])
    assert info["history_lost"] == 0 and info["history_refused"] == 0, info
    assert info["history_entries"] == wk.shards * wk.history, ("history_entries", info["history_entries"])
    assert info["table_slots"] == wk.shards * wk.slots, ("table_slots", info["table_slots"])
    if exact_arena is not None:
        assert info["arena_bytes_used"] == exact_arena, ("arena_bytes_used", info["arena_bytes_used"], exact_arena)
    assert info["arena_bytes_used"] >= live_bytes(export), ("arena_bytes_used", info["arena_bytes_used"])


def check_readers(rd, wk, exact_arena=None):
    """Every reader after a step. -> the export."""
    export = rd.export()
    check_export(export, wk)
    check_scans(rd, export, wk)
    check_hot(rd, export, wk)
    if wk.lc:
        check_hot(rd, export, wk, blocked=True)
        assert rd.lc_entries(wk.now) == wk.oc.local_cache.entry_count(wk.now), "local-cache entry_count"
    check_lookup(rd, wk)
    check_table_info(rd.table_info(), export, wk, exact_arena)
    return export


def expired_keys(export, floor):
    """The keys of the export whose every record (and local-cache entry) had expired at floor."""
    return {g[0][:2] for g in SC.groups_of(export) if all(floor > r[5] and r[6] <= floor for r in g)}


def check_op(op, a, got, pre, ia, post, ib, wk):
    """The call's own info. pre / post: the exports around it, ia / ib: table_info around it."""
    units = {}
    for g in SC.groups_of(pre):
        units.setdefault(g[0][0], []).append(g)
    before, after = {g[0][:2] for g in SC.groups_of(pre)}, {g[0][:2] for g in SC.groups_of(post)}
    if op in ("F_KEYS", "F_PREFIX"):
        want = [0] * len(a)
        for s in units:
            hit = [j for j, p in enumerate(a) if (s == p if op == "F_KEYS" else s.startswith(p))]
            if hit:
                want[hit[0]] += len(units[s])
        gone = {s for s in units if any(s == p if op == "F_KEYS" else s.startswith(p) for p in a)}
        assert got["removed"].tolist() == want, (op, got["removed"].tolist(), want)
        assert got["keys"] == sum(want) > 0 and (op == "F_PREFIX" or want[-1] == 0), (op, want)  # (the stem never seen)
        assert got["arena_bytes"] == sum(arena_bytes(s) * len(units[s]) for s in gone), (op, got["arena_bytes"])
        assert got["keys"] >= got["keys_with_history"] >= sum(len(g) > 1 for s in gone for g in units[s])
        assert got["slots_scanned"] == (wk.shards * wk.slots if op == "F_PREFIX" else 0)
        assert after == {k for k in before if k[0] not in gone}, op
        assert key_counts(post) == key_counts([r for r in pre if r[0] not in gone]), op  # every other record as it was
        for f in ("live_slots", "tombstones"):
            assert ib[f] == ia[f] + (got["keys"] if f == "tombstones" else -got["keys"]), (op, f)
        assert ib["arena_bytes_used"] == ia["arena_bytes_used"], op  # (they come back at the next sweep)
        return
    if op == "SWEEP":
        gone = expired_keys(pre, a)
        assert got == len(gone), (op, got, len(gone))
        assert after == before - gone, op
        assert key_counts(post) == key_counts([r for r in pre if r[:2] not in gone]), op
        return
    if op == "MIGRATE":
        # rl_import sends a key's older windows to the target's log "under its own horizon": a record may be
        # left out only where the log keeps none (DESIGN's hist_keep at J = 0): more than 8 windows behind
        # its key's newest window and dead, its EXPIRE and local-cache TTL, a divider before that window began
        newest = {g[0][:2]: g[-1] for g in SC.groups_of(pre)}
        assert after == before and {g[0][:2]: g[-1] for g in SC.groups_of(post)} == newest, (op, "the newest records")
        left_out = key_counts(pre)
        for r in post:
            assert left_out.get(r, 0) > 0, (op, "a record the source did not hold", r)
            left_out[r] -= 1
        for r in (r for r, n in left_out.items() if n):
            ws_new, d = newest[r[:2]][3], DIV[r[1]]
            assert ws_new - r[3] > 8 * d and max(r[5], r[6]) + d < ws_new, (op, "a record was lost", r, ws_new)
    else:
        assert key_counts(post) == key_counts(pre), (op, "the records changed")
    if op == "MIGRATE":
        assert got["keys"] == len(before) and got["records"] == len(pre), (op, got)
        assert got["chains_lost"] == 0 and got["time_floor"] == wk.floor, (op, got)
        return
    same = [f for f in ia if f not in ("table_slots", "tombstones", "history_entries")]
    if op in ("H_SMALL", "H_LARGE", "ARENA"):
        same += ["table_slots", "tombstones"]
    if op == "SNAPSHOT":  # (a fresh ctx: batches and decisions start again, history_appended is the image's entries)
        same = ["live_slots", "arena_bytes_used", "exact_stems", "history_slots", "history_lost", "history_refused"]
        assert ib["tombstones"] == ia["tombstones"], op
    for f in same:
        assert ib[f] == ia[f], (op, f, ia[f], ib[f])
    if op in ("T_SMALL", "T_LARGE"):
        assert got["keys"] == ia["live_slots"] and got["tombstones_dropped"] == ia["tombstones"], (op, got)
        assert got["slots_before"] == ia["table_slots"] and got["slots_after"] == ib["table_slots"], (op, got)
        assert got["log_entries_relinked"] >= len(pre) - len(before), (op, got)  # at least the exported older windows
    if op in ("H_SMALL", "H_LARGE"):  # test_gpu_relog._continue_across' identities
        assert got["entries_before"] == ia["history_entries"] and got["entries_after"] == ib["history_entries"], (op, got)
        assert got["chains"] == ia["history_slots"] and got["chains_lost"] == 0, (op, got)
        assert got["entries_kept"] >= got["chains"] and got["entries_kept"] >= len(pre) - len(before), (op, got)
        assert got["entries_kept"] + got["entries_dropped"] == got["written_before"] <= ia["history_appended"], (op, got)
        assert got["fill_max"] <= a // 64 and got["longest_chain"] >= 1, (op, got)


def first_difference(out, want, calls):
    """The first descriptor whose answer is not the oracle's, for a failure's report (or None)."""
    for c, (g, w) in enumerate(zip(out, want)):
        for d, (x, y) in enumerate(zip(g, w)):
            if x != y:
                r, lims, now = calls[c]
                return dict(call=c, descriptor=d, domain=r.domain, entries=r.descriptors[d].entries,
                            unit=lims[d].limit.unit, now=now, got=x, want=y)
    return None if len(out) == len(want) else dict(calls=len(out), want=len(want))
