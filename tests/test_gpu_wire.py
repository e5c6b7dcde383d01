"""GPU tests of the payload path (rl_do_limit_wire_async; k_wire_count,
k_wire_scan, k_wire_emit): serialized RateLimitRequest messages parsed on the
device. The host packer is the authority on every message's status, and the
packed path (rl_do_limit_requests_packed_async) on the batch rl_packer_pack +
rl_request_batch_pack make of the same messages, deferred and malformed ones
replaced by empty ones, is the reference for every output byte.

1. the C4 request streams through should_rate_limit_payloads_pipelined, twelve
   batches per rl_synchronize, against the oracle service in the order applied;
2. bytewise equality with the packed path in every output mode;
3. edge shapes (tile boundaries, empty messages, the extra wire cases, tiles past
   every LDS budget), one by one and all in flight;
4. bad messages between good ones: statuses, neighbours, guard bytes;
5. a decreasing msg_off fails its batch alone;
6. the three capacity failures at rl_synchronize;
7. host-detected errors enqueue nothing;
8. submission order against the other entry points, and completion through
   rl_batch_progress alone.
"""
import ctypes as C
import random
import time

import numpy as np
import pytest

from oracle import oracle as O
from oracle.config import OracleService, RateLimitConfig, StatsStore
from ratelimit_amd import abi
from ratelimit_amd.config import ConfigTree, RequestPacker, batch_arrays
from ratelimit_amd.limiter import Backend, GpuRateLimitService, PackedRequests, RedisError, WireRequests
from ratelimit_amd.packing import RuleInterner, pack_calls
import pbwire
import verdict_ref as V
import wire_cases as WC
from test_gpu_requests import FILES, SMALL, gen_requests, st_tuple
from test_gpu_requests_packed import DIVIDER, Flight, assert_same, backend_pair, guards_intact, table_state
from test_gpu_verdict import STREAMS

pytestmark = pytest.mark.gpu

INFLIGHT = abi.RL_REQUESTS_INFLIGHT
TILE = abi.RL_WIRE_TILE
OK, DEFERRED, MALFORMED = abi.RL_WIRE_OK, abi.RL_WIRE_DEFERRED, abi.RL_WIRE_MALFORMED


def encode(reqs):
    return [pbwire.encode_request(r, extra_unknown=(i % 4 == 0)) for i, r in enumerate(reqs)]


def cuts_of(seed, n, sizes=(1, 7, 64, 300)):
    rng = random.Random(seed * 7)
    cuts, i = [], 0
    while i < n:
        j = min(n, i + rng.choice(sizes))
        cuts.append((i, j))
        i = j
    return cuts


# ---- 1. the streams against the oracle service ------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2])
def test_gpu_wire_stream_matches_oracle_service(seed):
    p = STREAMS[seed]
    reqs, nows = gen_requests(seed, 1200)
    msgs = encode(reqs)
    cuts = cuts_of(seed, len(reqs))
    group = 12

    def deferred(q):  # a descriptor with a limit override
        return any(d.limit is not None for d in reqs[q].descriptors)

    # the order the service applies: per group of batches the requests without an override, then, batch by
    # batch, the deferred ones (those carrying one)
    order = []
    for g in range(0, len(cuts), group):
        part = cuts[g:g + group]
        for i, j in part:
            order += [q for q in range(i, j) if not deferred(q)]
        for i, j in part:
            order += [q for q in range(i, j) if deferred(q)]
    assert sorted(order) == list(range(len(reqs))) and order != sorted(order)
    assert sum(1 for q in order if deferred(q)) >= 20
    store = StatsStore()
    osvc = OracleService(RateLimitConfig(FILES, store), O.OracleFixedRateLimitCache(0.8, p["local_cache"], ""),
                         p["global_shadow"])
    want = {}
    for q in order:
        _, unl = osvc.construct_limits_to_check(reqs[q])
        ocode, osts, _ = osvc.should_rate_limit(reqs[q], nows[q])
        v = V.verdict(osts, unl, p["global_shadow"])
        assert v.code == ocode
        want[q] = (v, tuple(st_tuple(s) for s in osts))
    ostats = {k: list(v.as_tuple()) for k, v in store.by_key.items() if any(v.as_tuple())}

    # descriptors that hit a (key, window) the batch before them also hit (second halves out of order would
    # answer these differently)
    def keys(i, j):
        out = []
        for q in range(i, j):
            if deferred(q):
                continue
            for d, s in zip(reqs[q].descriptors, want[q][1]):
                if s[1] is not None:
                    out.append((reqs[q].domain, tuple(d.entries), nows[q] // DIVIDER[s[1][1]], s[1][1]))
        return out

    per_batch = [keys(i, j) for i, j in cuts]
    chained = sum(sum(1 for k in cur if k in prev) for prev, cur in zip(map(set, per_batch), per_batch[1:]))
    assert chained >= 100, chained
    svc = GpuRateLimitService(FILES, 0.8, p["local_cache"], "", global_shadow_mode=p["global_shadow"], **SMALL)
    got, shadow = [], 0
    try:
        for g in range(0, len(cuts), group):
            batches = [(msgs[i:j], nows[i:j]) for i, j in cuts[g:g + group]]
            for part, n in svc.should_rate_limit_payloads_pipelined(batches):
                got += part
                shadow += n
        assert svc.global_shadow_count == shadow
        assert len(got) == len(reqs)
        for q, g_ in enumerate(got):
            v, sts = want[q]
            assert (g_.code, g_.flags, g_.headers) == (v.code, v.flags, v.headers), q
            assert tuple(st_tuple(s) for s in g_.statuses) == sts, q
        assert dict(svc.stats) == ostats
        assert shadow == sum(v.shadow_inc for v, _ in want.values())
        assert (shadow > 0) == p["global_shadow"]
    finally:
        svc.close()


# ---- helpers for the raw entry point ----------------------------------------------------------

class WireFlight(Flight):
    """Wire batches and their guarded pinned buffers and outputs, kept alive until read."""

    def wire(self, msgs, nows, n_rules):
        probe = Backend.wire_batch(msgs, nows, None, n_rules)  # (pageable: the layout)
        size = int(probe.struct.buf_bytes)
        whole, buf = self.guarded(size, np.uint8)
        buf[:size] = probe.buf[:size]
        s = abi.RlWireBatch.from_buffer_copy(probe.struct)
        s.buf = buf.ctypes.data
        return s, buf, whole

    def submit_wire(self, be, msgs, nows, n_rules, n_desc, mode="both", global_shadow=False, desc_cap=None,
                    damage=None):
        """n_desc: the descriptors the outputs hold (the reference batch's count)."""
        s, buf, whole = self.wire(msgs, nows, n_rules)
        if damage:
            damage(s, buf)
        nq = len(msgs)
        p = PackedRequests(s, buf, nq, n_desc, n_rules)
        out, ver, guards = self.outputs(p, mode)
        wire = {}
        for k, n, dt in (("req_status", nq, np.uint8), ("desc_first", nq + 1, np.uint32), ("n_descriptors", 1, np.uint32)):
            w, wire[k] = self.guarded(n, dt)
            guards.append((w, wire[k]))
        keep = be.do_limit_wire_async(WireRequests(s, buf, nq, int(s.msgs_bytes)), wire, out, ver, global_shadow,
                                      n_desc if desc_cap is None else desc_cap)
        item = dict(p=p, out=out, ver=ver, wire=wire, guards=guards + [(whole, buf)], keep=keep, packed=bytes(buf))
        self.items.append(item)
        return item


def reference(pk, msgs, nows):
    """-> (the packer's status per message, the arrays of the batch the packer makes of the messages with
    every deferred or malformed one replaced by an empty one)."""
    st = np.array([WC.expect(pk, m)[0] for m in msgs], np.uint8)
    clean = [m if s == OK else b"" for m, s in zip(msgs, st)]
    a = batch_arrays(pk.pack(clean, nows))
    assert not a["override_flags"].any()
    return st, a


def assert_wire_same(item, ref, st, a, mode="both"):
    """item: a wire batch; ref: the packed path's item for the reference batch ``a``."""
    nq, n = len(st), len(a["req_idx"])
    assert item["wire"]["req_status"][:nq].tobytes() == st.tobytes()
    first = np.searchsorted(a["req_idx"], np.arange(nq + 1)).astype(np.uint32)
    assert item["wire"]["desc_first"][:nq + 1].tobytes() == first.tobytes()
    assert int(item["wire"]["n_descriptors"][0]) == n == ref["p"].n_descriptors
    nr = item["p"].n_rules
    if mode in ("out", "both"):
        for k in abi.REQUEST_RESULT_DTYPES:
            assert item["out"][k][:n].tobytes() == ref["out"][k][:n].tobytes(), k
        assert item["out"]["stats"][:nr * abi.RL_NUM_STATS].tobytes() == ref["out"]["stats"][:nr * abi.RL_NUM_STATS].tobytes()
    if mode in ("verdict", "both"):
        for k in abi.REQUEST_VERDICT_DTYPES:
            want = ref["ver"][k][:nq].copy()
            if k == "overall_code":
                assert (want != 0).all()
                want[st != OK] = 0  # no rl_code: a deferred or malformed request has no answer
            assert item["ver"][k][:nq].tobytes() == want.tobytes(), k
        assert ((item["ver"]["overall_code"][:nq] == 0) == (st != OK)).all()
        assert int(item["ver"]["global_shadow"][0]) == int(ref["ver"]["global_shadow"][0])
    guards_intact(item)
    guards_intact(ref)


class Pair:
    """Two ctxs with one hash seed: the wire path on one, the reference batches through the packed path on the other."""

    def __init__(self, **kw):
        (self.ref_be, self.be), self.it = backend_pair(**kw)
        self.n_rules = len(self.it.keys)
        self.fl = WireFlight()
        self.pk = RequestPacker(self.n_rules)

    def submit(self, msgs, nows, mode="both", global_shadow=False):
        st, a = reference(self.pk, msgs, nows)
        ref = self.fl.submit(self.ref_be, a, self.n_rules, mode, global_shadow)
        item = self.fl.submit_wire(self.be, msgs, nows, self.n_rules, len(a["req_idx"]), mode, global_shadow)
        return item, ref, st, a, mode

    def check(self, flight):
        self.be.synchronize()
        self.ref_be.synchronize()
        for item, ref, st, a, mode in flight:
            assert_wire_same(item, ref, st, a, mode)

    def close(self):
        self.pk.close()
        self.fl.close()
        self.ref_be.close()
        self.be.close()


# ---- 2. bytewise equality with the packed path ------------------------------------------------

def test_gpu_wire_equals_the_packed_path_bytewise():
    reqs, nows = gen_requests(2, 600)
    msgs = encode(reqs)
    pr = Pair()
    try:
        cuts = cuts_of(3, len(reqs))
        modes = ["out", "verdict", "both"]
        seen = np.zeros(3, np.int64)
        for g in range(0, len(cuts), 2 * INFLIGHT + 1):
            flight = [pr.submit(msgs[i:j], nows[i:j], modes[(g + b) % 3], True)
                      for b, (i, j) in enumerate(cuts[g:g + 2 * INFLIGHT + 1])]
            pr.check(flight)
            for f in flight:
                seen += np.bincount(f[2], minlength=3)
        assert seen[OK] > 500 and seen[DEFERRED] >= 10  # (the stream's overrides were deferred)
        assert table_state(pr.ref_be) == table_state(pr.be)
        assert pr.be.table_info()["decisions"] > 0
    finally:
        pr.close()


# ---- 3. the shapes at the kernels' edges -------------------------------------------------------

def edge_batches():
    """[(name, messages, nows)]"""
    out = []
    for nq in (0, 1, 255, 256, 257, 513):
        reqs, nows = gen_requests(100 + nq, nq)
        out.append(("n=%d" % nq, encode(reqs), nows))
    out.append(("only empty messages", [b""] * 300, [1_700_000_041] * 300))
    good, gnow = gen_requests(77, 40)
    good = encode(good)
    extras = WC.extra_cases()
    # every extra case between good messages
    msgs = []
    for i, (_, m) in enumerate(extras):
        msgs += [good[i % len(good)], m]
    out.append(("extra cases", msgs, [1_700_000_042] * len(msgs)))
    by = dict(extras)
    # tiles past each LDS budget: payload bytes (24 KB), entry bytes (16 KB), domains (4 KB), lengths (2048 entries)
    big = by["key_300_value_5000"]
    msgs = [big if q % 40 == 0 else good[q % len(good)] for q in range(300)]
    out.append(("payload and entry bytes past their budgets", msgs, [1_700_000_042] * len(msgs)))
    dom = pbwire.field_bytes(1, b"c4" + b"x" * 30)
    msgs = [dom + pbwire.field_bytes(2, pbwire.field_bytes(1, pbwire.field_bytes(1, b"k"))) for _ in range(300)]
    out.append(("domain bytes past their budget", msgs, [1_700_000_042] * len(msgs)))
    msgs = [by["entries_70"] if q % 6 == 0 else good[q % len(good)] for q in range(300)]
    out.append(("lengths past their budget", msgs, [1_700_000_042] * len(msgs)))
    # a 300-descriptor request inside a tile of small ones, in the test config's domain
    one = lambda i: O.Descriptor([("remote_address", "10.0.0.%d" % (i % 7))])  # noqa: E731
    rs = [O.RateLimitRequest("c4", [one(i)], 1) for i in range(100)] + \
         [O.RateLimitRequest("c4", [one(i) for i in range(300)], 2)] + \
         [O.RateLimitRequest("c4", [one(i)], 1) for i in range(200)]
    out.append(("300 descriptors among small requests", encode(rs), [1_700_000_043] * len(rs)))
    return out


@pytest.mark.parametrize("together", [False, True], ids=["one by one", "all in flight"])
def test_gpu_wire_edge_shapes_equal_the_packed_path(together):
    pr = Pair(max_batch=1 << 17, max_stem_bytes=1 << 22)
    try:
        flight = []
        for name, msgs, nows in edge_batches():
            f = pr.submit(msgs, nows)
            if not together:
                pr.check([f])
            flight.append(f)
        pr.check(flight)
        assert table_state(pr.ref_be) == table_state(pr.be)
    finally:
        pr.close()


# ---- 4. bad messages between good ones -------------------------------------------------------------

def test_gpu_wire_bad_messages_between_good_ones():
    reqs, nows = gen_requests(5, 400, p_override=0.0)
    good = encode(reqs)
    bad = WC.malformed() + WC.truncations(good[:2]) + WC.flips(200, msgs=good)
    pr = Pair()
    try:
        flight = []
        for b in range(0, len(bad), 150):
            part = bad[b:b + 150]
            msgs, ts = [], []
            for i, m in enumerate(part):
                msgs += [good[(b + i) % len(good)], m]
                ts += [nows[(b + i) % len(good)]] * 2
            ts.sort()
            flight.append(pr.submit(msgs, ts))
        pr.check(flight)
        st = np.concatenate([f[2] for f in flight])
        assert (st[0::2] == OK).all()  # the good neighbours
        assert (st[1::2] == MALFORMED).sum() >= 100 and (st[1::2] == OK).sum() >= 30
        assert table_state(pr.ref_be) == table_state(pr.be)
        assert pr.be.table_info()["decisions"] > 0
    finally:
        pr.close()


# ---- 5. a decreasing msg_off ------------------------------------------------------------------------

def test_gpu_wire_decreasing_msg_off_fails_alone():
    pr = Pair()
    try:
        batches = []
        for k in range(3):
            reqs, nows = gen_requests(200 + k, 300, p_override=0.0)
            batches.append((encode(reqs), nows))
        before = pr.submit(*batches[0])

        def damage(s, buf):
            off = buf[s.msg_off:s.msg_off + 4 * (s.n_requests + 1)].view(np.uint32)
            off[260], off[261] = off[261], off[260]  # (inside the second tile; the two ends stay)
            assert off[260] > off[261]

        n = sum(len(r.descriptors) for r in gen_requests(201, 300, p_override=0.0)[0])
        bad = pr.fl.submit_wire(pr.be, batches[1][0], batches[1][1], pr.n_rules, n, damage=damage)
        after = pr.submit(*batches[2])
        with pytest.raises(RedisError, match="RL_E_INVALID"):
            pr.be.synchronize()
        pr.check([before, after])  # (reported once: this synchronize succeeds)
        guards_intact(bad)
        assert table_state(pr.ref_be) == table_state(pr.be)
    finally:
        pr.close()


# ---- 6. capacity, known once the device has counted ------------------------------------------------

@pytest.mark.parametrize("case", ["desc_cap", "max_batch", "max_stem_bytes"])
def test_gpu_wire_capacity_fails_at_synchronize(case):
    one = lambda i: O.Descriptor([("remote_address", "10.0.0.%d" % (i % 9))])  # noqa: E731
    mid = encode([O.RateLimitRequest("c4", [one(i), one(i + 1)], 1) for i in range(100)])  # 200 descriptors
    n, ent_bytes = 200, sum(2 * len("remote_address_10.0.0.0_") for _ in range(100))
    small, snow = gen_requests(9, 12, p_override=0.0)
    small = encode(small)
    kw = {"max_batch": dict(max_batch=n - 1), "max_stem_bytes": dict(max_stem_bytes=ent_bytes - 1)}.get(case, {})
    pr = Pair(**kw)
    try:
        st, a = reference(pr.pk, mid, [1_700_000_040] * 100)
        assert len(a["req_idx"]) == n and int(a["desc_off"][-1]) == ent_bytes and (st == OK).all()
        before = pr.submit(small, snow)
        bad = pr.fl.submit_wire(pr.be, mid, [1_700_000_040] * 100, pr.n_rules, n,
                                desc_cap=n - 1 if case == "desc_cap" else n)
        after = pr.submit(small, snow)
        with pytest.raises(RedisError, match="RL_E_CAPACITY"):
            pr.be.synchronize()
        pr.check([before, after])
        guards_intact(bad)
        assert table_state(pr.ref_be) == table_state(pr.be)
        if case == "desc_cap":  # counts only with out: the same batch, verdict only, goes through
            pr.check([pr.submit(mid, [1_700_000_040] * 100, "verdict")])
    finally:
        pr.close()


# ---- 7. host-detected errors ------------------------------------------------------------------------

def test_gpu_wire_host_detected_errors_enqueue_nothing():
    it = RuleInterner()
    tree = ConfigTree.from_yaml(FILES, "", it)
    be = Backend(0.8, True, **SMALL)
    bare = Backend(0.8, True, **SMALL)
    two = Backend(0.8, True, n_shards=2, shard_devices=[0, 0], hash_seed=5, **SMALL)
    fl = WireFlight()
    try:
        for b in (be, two):
            b.load_config(tree)
        reqs, nows = gen_requests(41, 300, p_override=0.0)
        msgs = encode(reqs)
        n = sum(len(r.descriptors) for r in reqs)
        s, buf, whole = fl.wire(msgs, nows, len(it.keys))
        p = PackedRequests(s, buf, len(msgs), n, len(it.keys))
        out, ver, guards = fl.outputs(p, "both")
        w_status, status = fl.guarded(len(msgs), np.uint8)
        fill = [bytes(wh.view(np.uint8)) for wh, _ in guards] + [bytes(w_status.view(np.uint8))]

        def call(b, s, out=out, ver=ver, opts=0, wire=True, status=status, reserved=0):
            r = v = wr = None
            if out is not None:
                r = abi.RlRequestResult()
                for k in out:
                    setattr(r, k, abi.ptr(out[k]))
            if ver is not None:
                v = abi.RlRequestVerdict()
                for k in ver:
                    setattr(v, k, abi.ptr(ver[k]))
            if wire:
                wr = abi.RlWireResult()
                wr.req_status = abi.ptr(status)
                wr.desc_cap, wr.reserved = n, reserved
            return b.L.rl_do_limit_wire_async(b.ctx, C.byref(s) if s is not None else None,
                                              C.byref(wr) if wr else None, C.byref(r) if r else None, opts,
                                              C.byref(v) if v else None)

        def changed(**fields):
            c = abi.RlWireBatch.from_buffer_copy(s)
            for k, x in fields.items():
                setattr(c, k, x)
            return c

        B = int(s.buf_bytes)
        sub0 = be.batch_progress()[0]
        assert call(be, None) == abi.RL_E_INVALID
        assert call(be, changed(), wire=False) == abi.RL_E_INVALID
        assert call(be, changed(), status=None) == abi.RL_E_INVALID
        assert call(be, changed(), out=None, ver=None) == abi.RL_E_INVALID      # both outputs NULL
        for k in ("msg_off", "now", "msgs"):
            assert call(be, changed(**{k: B + 4})) == abi.RL_E_INVALID, k       # outside buf
            assert call(be, changed(**{k: getattr(s, k) + 2})) == abi.RL_E_INVALID, k  # not 4-byte aligned
        assert call(be, changed(buf_bytes=B - 4)) == abi.RL_E_INVALID            # the payload section cut short
        assert call(be, changed(msgs_bytes=s.msgs_bytes - 1)) == abi.RL_E_INVALID  # msg_off's end
        off = buf[s.msg_off:s.msg_off + 4].view(np.uint32)
        off[0] = 1
        assert call(be, changed()) == abi.RL_E_INVALID                           # msg_off[0] != 0
        off[0] = 0
        assert call(be, changed(), reserved=1) == abi.RL_E_INVALID
        assert call(be, changed(), opts=2) == abi.RL_E_INVALID                  # unknown opts bit
        assert call(be, changed(n_rules=SMALL["max_rules"] + 1)) == abi.RL_E_CAPACITY
        big = fl.wire([b""] * (SMALL["max_batch"] + 1), [7] * (SMALL["max_batch"] + 1), 1)[0]
        assert call(be, big) == abi.RL_E_CAPACITY                               # n_requests > max_requests
        assert be.batch_progress()[0] == sub0
        sub0 = bare.batch_progress()[0]
        assert call(bare, changed()) == abi.RL_E_INVALID                        # no config loaded
        assert b"configuration" in bare.L.rl_last_error(bare.ctx)
        assert bare.batch_progress()[0] == sub0
        assert call(two, changed()) == abi.RL_E_INVALID                         # single-shard ctxs only
        # nothing ran: the outputs keep their fill, the table is empty, and the good batch still goes through
        assert fill == [bytes(wh.view(np.uint8)) for wh, _ in guards] + [bytes(w_status.view(np.uint8))]
        assert be.table_info()["decisions"] == 0 and be.table_info()["live_slots"] == 0
        sub0 = be.batch_progress()[0]
        assert call(be, changed()) == abi.RL_OK
        assert be.batch_progress()[0] == sub0 + 1
        be.synchronize()
        assert be.table_info()["decisions"] > 0 and (status == OK).all()
    finally:
        fl.close()
        for b in (be, bare, two):
            b.close()


# ---- 8. order and completion -----------------------------------------------------------------------

def test_gpu_wire_interleaves_in_submission_order():
    from ratelimit_amd.config import pack_requests
    it = RuleInterner()
    tree = ConfigTree.from_yaml(FILES, "", it)
    be = Backend(0.8, False, **SMALL)
    fl = WireFlight()
    try:
        be.load_config(tree)
        now = 1_700_003_000
        tenants = ["t%d" % i for i in range(20)]
        reqs = [O.RateLimitRequest("c4", [O.Descriptor([("tenant", t)])], 1 + i % 3) for i, t in enumerate(tenants)]
        msgs = encode(reqs)
        a = pack_requests(reqs, [now] * len(reqs), it)
        lim = O.new_rate_limit(40, O.HOUR, "c4.tenant")
        pb = pack_calls([(O.RateLimitRequest("c4", [O.Descriptor([("tenant", t)])], 5), [lim], now) for t in tenants],
                        "", RuleInterner())
        first = fl.submit_wire(be, msgs, [now] * 20, len(it.keys), 20)
        mid = be.do_limit_packed(pb)                       # rl_do_limit on the same keys
        second = fl.submit(be, a, len(it.keys))            # the packed path
        third = fl.submit_wire(be, msgs, [now] * 20, len(it.keys), 20)
        off = pb.arrays["stem_off"]
        stems = [bytes(pb.arrays["stem_bytes"][off[i]:off[i + 1]]) for i in range(len(tenants))]
        look = be.lookup(stems, [O.HOUR] * len(stems), [now] * len(stems))  # completes the pending batches first
        h = np.array([1 + i % 3 for i in range(len(tenants))])
        assert list(mid["limit_remaining"]) == list(40 - h - 5)
        assert list(look["count"]) == list(3 * h + 5) and look["found"].all()
        be.synchronize()
        assert list(first["out"]["limit_remaining"][:20]) == list(40 - h)
        assert list(second["out"]["limit_remaining"][:20]) == list(40 - 2 * h - 5)
        assert list(third["out"]["limit_remaining"][:20]) == list(40 - 3 * h - 5)
        assert (first["out"]["match"][:20] == abi.RL_MATCH_LIMIT).all()
        assert (first["wire"]["req_status"][:20] == OK).all() and int(third["wire"]["n_descriptors"][0]) == 20
    finally:
        fl.close()
        be.close()


def test_gpu_wire_progress_completes_the_flight():
    pr = Pair()
    try:
        flight = []
        for k in range(2 * INFLIGHT + 1):  # more than the ring holds
            reqs, nows = gen_requests(50 + k, 200)
            flight.append(pr.submit(encode(reqs), nows))
        pr.ref_be.synchronize()
        deadline = time.monotonic() + 10
        while True:
            sub, done = pr.be.batch_progress()
            assert sub == len(flight)
            if done == sub:
                break
            assert time.monotonic() < deadline, (sub, done)
            time.sleep(0.001)
        for item, ref, st, a, mode in flight:  # (no rl_synchronize on the wire ctx so far)
            assert_wire_same(item, ref, st, a, mode)
        pr.be.synchronize()
        assert table_state(pr.ref_be) == table_state(pr.be)
    finally:
        pr.close()
