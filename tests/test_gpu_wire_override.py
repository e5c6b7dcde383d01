"""Descriptor limit overrides answered on the wire path: the override stats
keys interned on the GPU (rl_override_rules_enable). The streams against the
oracle service in arrival order, the raw entry points bytewise against the
packed path on the packer's batch (override rule ids compared by key name),
the identity of keys, first sight under concurrency, the table's limits and the
errors at the call."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from oracle.config import OracleService, RateLimitConfig, StatsStore
from ratelimit_amd import abi
from ratelimit_amd.config import RequestPacker, batch_arrays
from ratelimit_amd.limiter import Backend, GpuRateLimitService, PackedRequests, PinnedArena, RedisError, WireRequests
import override_cases as OC
import verdict_ref as V
from test_gpu_requests import FILES, SMALL, gen_requests, st_tuple
from test_gpu_requests_packed import backend_pair, guards_intact, table_state
from test_gpu_verdict import STREAMS
from test_gpu_wire import WireFlight, cuts_of, encode

pytestmark = pytest.mark.gpu

INFLIGHT = abi.RL_REQUESTS_INFLIGHT
OK, DEFERRED, MALFORMED = abi.RL_WIRE_OK, abi.RL_WIRE_DEFERRED, abi.RL_WIRE_MALFORMED
HK = (b"x-ratelimit-limit", b"x-ratelimit-remaining", b"x-ratelimit-reset")
NOW = 1_700_000_041


def has_override(r):
    return any(d.limit is not None for d in r.descriptors)


# ---- 1. the stream against the oracle service, in arrival order --------------------------------

def _oracle(reqs, nows, order, p):
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
    return want, {k: list(v.as_tuple()) for k, v in store.by_key.items() if any(v.as_tuple())}


def _same_as_oracle(got, want):
    assert len(got) == len(want)
    for q, g_ in enumerate(got):
        v, sts = want[q]
        assert (g_.code, g_.flags, g_.headers) == (v.code, v.flags, v.headers), q
        assert tuple(st_tuple(s) for s in g_.statuses) == sts, q


@pytest.mark.parametrize("seed", [1, 2])
def test_gpu_override_stream_matches_oracle_service_in_arrival_order(seed):
    p = STREAMS[seed]
    reqs, nows = gen_requests(seed, 600, p_override=0.2)
    msgs = encode(reqs)
    cuts = cuts_of(seed, len(reqs))
    batches = [(msgs[i:j], nows[i:j]) for i, j in cuts]
    n_ov = sum(1 for r in reqs if has_override(r))
    assert n_ov >= 100 and len(cuts) > INFLIGHT
    # override and config requests share cache keys: the same (domain, entries) with and without a limit
    with_ov = {(r.domain, tuple(d.entries)) for r in reqs for d in r.descriptors if d.limit is not None}
    without = {(r.domain, tuple(d.entries)) for r in reqs for d in r.descriptors if d.limit is None}
    assert len(with_ov & without) >= 20
    arrival, ostats = _oracle(reqs, nows, range(len(reqs)), p)
    svc = GpuRateLimitService(FILES, 0.8, p["local_cache"], "", global_shadow_mode=p["global_shadow"],
                              device_overrides=True, override_capacity=512, **SMALL)
    try:
        got, shadow = [], 0
        for part, n in svc.should_rate_limit_payloads_pipelined(batches):  # all cuts in flight
            got += part
            shadow += n
        _same_as_oracle(got, arrival)
        assert dict(svc.stats) == ostats
        assert shadow == sum(v.shadow_inc for v, _ in arrival.values()) == svc.global_shadow_count
        info = svc.backend.override_rules_info()
        keys = {"%s.%s" % (r.domain, ".".join(k + ("_" + v if v else "") for k, v in d.entries))
                for r in reqs for d in r.descriptors if d.limit is not None}
        assert info["rules"] == len(keys) and info["deferred_full"] == 0
        assert {k.decode() for k in svc.backend.override_rule_keys()} == keys
        # nothing with a (valid-unit) override is deferred: rules == the key count with deferred_full == 0
        # above, and directly, the statuses of the first 300 messages submitted once more
        arena = PinnedArena()
        try:
            wb = svc.backend.wire_batch(msgs[:300], nows[:300], arena, svc._wire_rules())
            wire = {"req_status": arena.array(300, np.uint8)}
            ver = {"overall_code": arena.array(300, np.uint8)}
            keep = svc.backend.do_limit_wire_async(wb, wire, None, ver)
            svc.backend.synchronize()
            assert (wire["req_status"] == OK).all() and keep is not None
        finally:
            arena.close()
    finally:
        svc.close()
    # the same stream through a service without the feature: the deferral path is what it was (the messages
    # with an override take effect after every batch of the call, batch by batch)
    order = [q for i, j in cuts for q in range(i, j) if not has_override(reqs[q])] + \
            [q for i, j in cuts for q in range(i, j) if has_override(reqs[q])]
    late, lstats = _oracle(reqs, nows, order, p)
    assert any(late[q] != arrival[q] for q in range(len(reqs)))  # (the order is observable on this stream)
    svc = GpuRateLimitService(FILES, 0.8, p["local_cache"], "", global_shadow_mode=p["global_shadow"], **SMALL)
    try:
        got = [g for part, _ in svc.should_rate_limit_payloads_pipelined(batches) for g in part]
        _same_as_oracle(got, late)
        assert dict(svc.stats) == lstats
    finally:
        svc.close()


def test_gpu_override_responses_match_oracle_service_in_arrival_order():
    """should_rate_limit_responses_pipelined with device_overrides: payload bytes in, payload bytes out."""
    p = STREAMS[1]
    reqs, nows = gen_requests(3, 300, p_override=0.2)
    msgs = encode(reqs)
    batches = [(msgs[i:j], nows[i:j]) for i, j in cuts_of(3, len(reqs))]
    arrival, ostats = _oracle(reqs, nows, range(len(reqs)), p)
    svc = GpuRateLimitService(FILES, 0.8, p["local_cache"], "", header_keys=HK, device_overrides=True, **SMALL)
    ref = GpuRateLimitService(FILES, 0.8, p["local_cache"], "", header_keys=HK, **SMALL)
    try:
        got = [r for part, _ in svc.should_rate_limit_responses_pipelined(batches) for r in part]
        # the host path, request by request in arrival order, serialized by rl_response_serialize
        want = []
        for m, now in zip(msgs, nows):
            want += ref.should_rate_limit_responses_pipelined([([m], [now])])[0][0]
        assert got == want
        assert dict(svc.stats) == ostats == dict(ref.stats)
    finally:
        svc.close()
        ref.close()


# ---- the raw entry points against the packed path ----------------------------------------------

class OvPair:
    """Two ctxs with one hash seed: the wire path with device-interned override rules on one, the packer's
    batch of the same messages through the packed path on the other (built once the wire statuses are known:
    every message that is not RL_WIRE_OK is replaced by an empty one)."""

    def __init__(self, capacity=512, key_bytes=0, rule_room=None, **kw):
        (self.ref_be, self.be), self.it = backend_pair(**kw)
        self.nc = len(self.it.keys)
        self.be.enable_override_rules(self.nc, capacity, key_bytes)
        self.n_rules = self.nc + (capacity if rule_room is None else rule_room)
        self.fl = WireFlight()
        self.pk = RequestPacker(self.nc)
        self.alone = RequestPacker(self.nc)
        self.ids = {}  # key bytes -> the id the device gave it, as first seen in an output

    def classify(self, msgs):
        """-> per message: MALFORMED, OK (no override), DEFERRED (a unit outside 1..4 or a key over 65535
        bytes) or "ov" (valid overrides); and the descriptors of the well-formed ones."""
        kinds, n = [], 0
        for m in msgs:
            info = OC.packer_overrides(self.alone, m)
            if info is None:
                kinds.append(MALFORMED)
                continue
            n += info[0]
            if not info[1]:
                kinds.append(OK)
            elif any(not 1 <= u <= 4 or len(k) > 65535 for _, _, u, k in info[1]) or \
                    len(info[1]) * (info[2] + 1) > 16 * len(m):  # (a long domain repeated over many overrides)
                kinds.append(DEFERRED)
            else:
                kinds.append("ov")
        return kinds, n

    def submit(self, msgs, nows, global_shadow=False):
        kinds, cap = self.classify(msgs)
        cap = max(cap, 1)
        fl, nq = self.fl, len(msgs)
        s, buf, whole = fl.wire(msgs, nows, self.n_rules)
        p = PackedRequests(s, buf, nq, cap, self.n_rules)
        out, ver, guards = fl.outputs(p, "both")
        wire = {}
        for k, n, dt in (("req_status", nq, np.uint8), ("desc_first", nq + 1, np.uint32), ("n_descriptors", 1, np.uint32)):
            w, wire[k] = fl.guarded(n, dt)
            guards.append((w, wire[k]))
        resp = {}
        for k, n, dt in (("bytes", Backend.response_bound(nq, cap, HK), np.uint8), ("resp_off", nq + 1, np.uint32)):
            w, resp[k] = fl.guarded(n, dt)
            guards.append((w, resp[k]))
        keep = self.be.do_limit_wire_respond_async(WireRequests(s, buf, nq, int(s.msgs_bytes)), wire, out, ver, resp, HK,
                                                   global_shadow, cap)
        item = dict(p=p, out=out, ver=ver, wire=wire, resp=resp, guards=guards + [(whole, buf)], keep=keep,
                    packed=bytes(buf), msgs=msgs, nows=nows, kinds=kinds, gs=global_shadow)
        fl.items.append(item)
        return item

    def check(self, items, strict=True):
        """strict: every message with valid overrides must be RL_WIRE_OK (else OK or DEFERRED)."""
        self.be.synchronize()
        dev = self.be.override_rule_keys()
        refs = []
        for it in items:
            nq = len(it["msgs"])
            st = it["wire"]["req_status"][:nq].copy()
            for q, kind in enumerate(it["kinds"]):
                if kind == "ov":
                    assert st[q] == OK or (not strict and st[q] == DEFERRED), (q, st[q])
                else:
                    assert st[q] == kind, (q, st[q], kind)
            clean = [m if s == OK else b"" for m, s in zip(it["msgs"], st)]
            a = batch_arrays(self.pk.pack(clean, it["nows"]))
            refs.append((st, a, self.fl.submit(self.ref_be, a, max(self.pk.rules(), 1), "both", it["gs"])))
        self.ref_be.synchronize()
        for it, (st, a, ref) in zip(items, refs):
            self.same(it, st, a, ref, dev)
        return [st for st, _, _ in refs]

    def name(self, dev, r):
        return dev[r - self.nc] if r >= self.nc else self.it.keys[r].encode()

    def ref_name(self, r):
        return self.pk._lib.rl_packer_rule_key(self.pk.h, r) if r >= self.nc else self.it.keys[r].encode()

    def same(self, it, st, a, ref, dev):
        nq, n = len(st), len(a["req_idx"])
        first = np.searchsorted(a["req_idx"], np.arange(nq + 1)).astype(np.uint32)
        assert it["wire"]["desc_first"][:nq + 1].tobytes() == first.tobytes()
        assert int(it["wire"]["n_descriptors"][0]) == n
        for k in abi.REQUEST_RESULT_DTYPES:
            if k != "rule_id":
                assert it["out"][k][:n].tobytes() == ref["out"][k][:n].tobytes(), k
        got_r, ref_r = it["out"]["rule_id"][:n], ref["out"]["rule_id"][:n]
        ov = a["override_flags"].astype(bool) & (it["out"]["match"][:n] == abi.RL_MATCH_LIMIT)
        assert (got_r[~ov] == ref_r[~ov]).all()
        for d in np.nonzero(ov)[0]:
            g, r = int(got_r[d]), int(ref_r[d])
            assert self.nc <= g < self.n_rules and r >= self.nc
            key = OC.key_of(a, d)
            assert self.name(dev, g) == key == self.ref_name(r)
            assert self.ids.setdefault(key, g) == g  # a key keeps its id
        # the stats rows, by key name
        def rows(stats, nr, name):
            t = stats[:nr * abi.RL_NUM_STATS].reshape(-1, abi.RL_NUM_STATS)
            return {name(int(r)): t[r].tolist() for r in np.nonzero(t.any(axis=1))[0]}
        assert rows(it["out"]["stats"], self.n_rules, lambda r: self.name(dev, r)) == \
            rows(ref["out"]["stats"], ref["p"].n_rules, self.ref_name)
        for k in abi.REQUEST_VERDICT_DTYPES:
            want = ref["ver"][k][:nq].copy()
            if k == "overall_code":
                want[st != OK] = 0
            assert it["ver"][k][:nq].tobytes() == want.tobytes(), k
        assert int(it["ver"]["global_shadow"][0]) == int(ref["ver"]["global_shadow"][0])
        # the responses: rl_response_serialize of those answers
        res = {k: it["out"][k][:n] for k in abi.REQUEST_RESULT_DTYPES}
        vd = {k: it["ver"][k][:nq] for k in abi.REQUEST_VERDICT_DTYPES}
        raw, off = Backend.response_serialize(first, st, res, vd, HK)
        assert it["resp"]["resp_off"][:nq + 1].tobytes() == off.tobytes()
        assert it["resp"]["bytes"][:int(off[nq])].tobytes() == raw.tobytes()
        guards_intact(it)
        guards_intact(ref)

    def close(self):
        self.pk.close()
        self.alone.close()
        self.fl.close()
        self.ref_be.close()
        self.be.close()


def ov_msg(key, value, rpu=5, unit=2, domain=b"c4", hits=1, extra=()):
    """One request: a descriptor (key, value) with a limit, after the descriptors of ``extra``."""
    return OC.message(domain, *extra, OC.desc(OC.entry(key, value), OC.limit(rpu, unit)), hits=hits)


# ---- 2. bytewise against the packed path --------------------------------------------------------

def test_gpu_override_wire_equals_the_packed_path_bytewise():
    reqs, nows = gen_requests(2, 600, p_override=0.2)
    msgs = encode(reqs)
    pr = OvPair()
    try:
        cuts = cuts_of(3, len(reqs))
        n_ov = 0
        for g in range(0, len(cuts), 2 * INFLIGHT + 1):
            flight = [pr.submit(msgs[i:j], nows[i:j], True) for i, j in cuts[g:g + 2 * INFLIGHT + 1]]
            for it, st in zip(flight, pr.check(flight)):
                assert (st == OK).all()
                n_ov += it["kinds"].count("ov")
        assert n_ov >= 100
        assert table_state(pr.ref_be) == table_state(pr.be)
        assert pr.be.table_info()["decisions"] > 0
        # the names are exactly the packer's key set, one id each
        info = pr.be.override_rules_info()
        want = {pr.ref_name(r) for r in range(pr.nc, pr.pk.rules())}
        dev = pr.be.override_rule_keys()
        assert len(dev) == info["rules"] == len(want) and set(dev) == want
        assert info["deferred_full"] == 0 and info["key_bytes_used"] == sum(len(k) for k in dev)
    finally:
        pr.close()


# ---- 3. identity -------------------------------------------------------------------------------

def test_gpu_override_identity_is_the_keys_bytes():
    plain, pnow = gen_requests(9, 60, p_override=0.0)
    plain = encode(plain)
    pr = OvPair()
    try:
        first = [ov_msg(b"a_b", b""), ov_msg(b"a", b"b"),              # one stats key
                 ov_msg(b"remote_address", b"10.0.0.1"), ov_msg(b"remote_address", b"10.0.0.2"),  # one byte apart
                 ov_msg(b"a", b"b", domain=b"c5"), ov_msg(b"a", b"b", domain=b"test-domain"),
                 ov_msg(b"tenant", b"t1", extra=[OC.desc(OC.entry(b"a_b", b""), OC.limit(9, 1))])]
        it1 = pr.submit(first + plain[:20], [NOW] * (len(first) + 20))
        pr.check([it1])
        dev = pr.be.override_rule_keys()
        assert sorted(dev) == sorted([b"c4.a_b", b"c4.remote_address_10.0.0.1", b"c4.remote_address_10.0.0.2",
                                      b"c5.a_b", b"test-domain.a_b", b"c4.tenant_t1"])
        rid = it1["out"]["rule_id"]
        assert rid[0] == rid[1] == rid[6] and len({int(rid[0]), int(rid[2]), int(rid[3]), int(rid[5]), int(rid[7])}) == 5
        ids = dict(pr.ids)  # (the keys whose descriptors matched: c5 is no domain of the config)
        assert ids[b"c4.a_b"] == int(rid[0]) and sorted(ids) == sorted(set(dev) - {b"c5.a_b"})
        # batches 2..5 bring new keys; the old ones keep their ids, in flight and after a resize
        flight = [pr.submit([ov_msg(b"k%d" % b, b"v%d" % i) for i in range(10)] + plain[20 + b:30 + b] +
                            ([ov_msg(b"a", b"b"), ov_msg(b"remote_address", b"10.0.0.2")] if b == 5 else []),
                            [NOW + b] * (22 if b == 5 else 20)) for b in range(2, 6)]
        pr.check(flight)
        pr.be.resize(1 << 17)
        pr.ref_be.resize(1 << 17)
        it6 = pr.submit(first, [NOW + 7] * len(first))
        pr.check([it6])
        assert it6["out"]["rule_id"][:8].tobytes() == rid[:8].tobytes()
        for k, v in ids.items():
            assert pr.ids[k] == v
        info = pr.be.override_rules_info()
        assert info["rules"] == 6 + 40 == len(pr.be.override_rule_keys())
        assert pr.be.override_rule_keys(pr.nc, 6) == dev  # (ids in the order of first sight: the first six)
        assert table_state(pr.ref_be) == table_state(pr.be)
    finally:
        pr.close()


# ---- 4. concurrent first sight ---------------------------------------------------------------------

@pytest.mark.parametrize("distinct", [1, 256])
def test_gpu_override_concurrent_first_sight(distinct):
    pr = OvPair()
    try:
        msgs = [ov_msg(b"remote_address", b"9.9.9.%d" % (i % distinct), rpu=1000) for i in range(300)]
        flight = [pr.submit(msgs, [NOW] * 300) for _ in range(INFLIGHT)]
        for st in pr.check(flight):
            assert (st == OK).all()  # (a spurious deferral is a failure)
        info = pr.be.override_rules_info()
        assert info["rules"] == distinct and info["deferred_full"] == 0
        assert sorted(pr.be.override_rule_keys()) == sorted({b"c4.remote_address_9.9.9.%d" % i for i in range(distinct)})
        assert table_state(pr.ref_be) == table_state(pr.be)
    finally:
        pr.close()


# ---- 5. limits -------------------------------------------------------------------------------------

def _limit_batches():
    plain, _ = gen_requests(12, 90, p_override=0.0)
    plain = encode(plain)
    out = []
    for b in range(3):
        msgs = []
        for i in range(30):
            msgs.append(plain[30 * b + i])
            msgs.append(ov_msg(b"user", b"u%02d" % ((7 * b + i) % 20), rpu=3 + i % 4, unit=1 + i % 4))
        msgs.append(ov_msg(b"user", b"u00", unit=5))   # units outside 1..4: the host's
        msgs.append(ov_msg(b"user", b"u01", unit=0))
        out.append((msgs, [NOW + b] * len(msgs)))
    return out


@pytest.mark.parametrize("case", ["capacity", "arena", "n_rules"])
def test_gpu_override_limits_defer_and_never_fail(case):
    kw = {"capacity": dict(capacity=8), "arena": dict(capacity=64, key_bytes=50),
          "n_rules": dict(capacity=64, rule_room=3)}[case]
    pr = OvPair(**kw)
    try:
        flight = [pr.submit(m, n) for m, n in _limit_batches()]
        sts = pr.check(flight, strict=False)  # (every OK message equals the packed path's answer; guards intact)
        n_ok = sum(int(st[q] == OK) for it, st in zip(flight, sts) for q, k in enumerate(it["kinds"]) if k == "ov")
        n_def = sum(int(st[q] == DEFERRED) for it, st in zip(flight, sts) for q, k in enumerate(it["kinds"]) if k == "ov")
        info = pr.be.override_rules_info()
        assert n_ok > 0 and n_def > 0 and info["deferred_full"] == n_def
        dev = pr.be.override_rule_keys()
        assert len(dev) == info["rules"] == len(set(dev))
        if case == "capacity":
            assert info["rules"] == 8 == info["capacity"]
        elif case == "arena":
            assert info["key_bytes_cap"] == 50 and info["key_bytes_used"] == sum(len(k) for k in dev) <= 50
            assert 0 < info["rules"] == 50 // len(b"c4.user_u00")
        else:  # ids past n_rules are handed out and never used by this batch
            assert info["rules"] == 20
            assert all(g < pr.nc + 3 for g in pr.ids.values()) and len(pr.ids) == 3
        assert table_state(pr.ref_be) == table_state(pr.be)
    finally:
        pr.close()


def test_gpu_override_long_key_and_bad_unit_are_deferred_alone():
    plain, _ = gen_requests(13, 40, p_override=0.0)
    plain = encode(plain)
    pr = OvPair(key_bytes=1 << 17, max_batch=1 << 17, max_stem_bytes=1 << 22)
    try:
        long_key = ov_msg(b"K" * 40000, b"V" * 30000)  # (each item within 65535, the key past it)
        edge = OC.message(b"c4", OC.desc(OC.entry(b"K" * 32760, b"V" * 32770), OC.limit(5, 1)))  # 3 + 32760 + 1 + 32770
        assert len(b"c4." + b"K" * 32760 + b"_" + b"V" * 32770) == 65534
        msgs = plain[:10] + [long_key] + plain[10:20] + [ov_msg(b"user", b"u1", unit=7), edge,
                                                         ov_msg(b"user", b"u1", unit=255), ov_msg(b"user", b"u1")]
        it = pr.submit(msgs, [NOW] * len(msgs))
        assert it["kinds"][10] == DEFERRED and it["kinds"][21] == DEFERRED and it["kinds"][22] == "ov"
        (st,) = pr.check([it])
        assert st.tolist() == [OK] * 10 + [DEFERRED] + [OK] * 10 + [DEFERRED, OK, DEFERRED, OK]
        info = pr.be.override_rules_info()
        assert info["rules"] == 2 and info["deferred_full"] == 0  # (not the table's doing)
        # a long domain in front of many small overrides: every key repeats the domain, so such a message
        # is the host's; one override fewer than the bound allows is answered here
        def many(n_ov, dom):
            return OC.message(dom, *[OC.desc(OC.entry(b"k", b"%d" % (i % 10)), OC.limit(5, 1)) for i in range(n_ov)])
        dom = b"c4" + b"x" * 1998
        over, under = many(40, dom), many(16, dom)
        assert 40 * 2001 > 16 * len(over) and 16 * 2001 <= 16 * len(under)
        it = pr.submit(plain[20:25] + [over, under] + plain[25:30], [NOW + 1] * 12)
        assert it["kinds"][5] == DEFERRED and it["kinds"][6] == "ov"
        (st,) = pr.check([it])
        assert st.tolist() == [OK] * 5 + [DEFERRED, OK] + [OK] * 5
        assert pr.be.override_rules_info()["rules"] == 2 + 10
    finally:
        pr.close()


# ---- 6. errors at the call -------------------------------------------------------------------------

def _enable_raw(be, first, capacity, key_bytes=0, reserved=(0, 0, 0, 0)):
    cfg = abi.RlOverrideRulesConfig()
    cfg.first_rule, cfg.capacity, cfg.key_bytes = first, capacity, key_bytes
    for i, r in enumerate(reserved):
        cfg.reserved[i] = r
    return be.L.rl_override_rules_enable(be.ctx, C.byref(cfg))


def test_gpu_override_errors_at_the_call():
    from ratelimit_amd.sharded import loopback_id
    (ref_be, be), it = backend_pair()
    ref_be.close()
    fl = WireFlight()
    try:
        nc, mr = len(it.keys), SMALL["max_rules"]
        # a ctx without the feature: the getters refuse, a limit is deferred as ever
        info = abi.RlOverrideRulesInfo()
        off = np.zeros(2, np.uint32)
        assert be.L.rl_override_rules_info_get(be.ctx, C.byref(info)) == abi.RL_E_INVALID
        assert be.L.rl_override_rule_keys(be.ctx, nc, 0, None, 0, abi.ptr(off), None) == abi.RL_E_INVALID
        item = fl.submit_wire(be, [ov_msg(b"user", b"u1"), OC.message(b"c4", OC.desc(OC.entry(b"user", b"u1")))],
                              [NOW, NOW], nc, 2)
        be.synchronize()
        assert item["wire"]["req_status"][:2].tolist() == [DEFERRED, OK]
        # every refused configuration leaves the feature off
        for i in range(4):
            assert _enable_raw(be, nc, 8, reserved=[int(j == i) for j in range(4)]) == abi.RL_E_INVALID
        assert _enable_raw(be, nc, 0) == abi.RL_E_INVALID
        assert _enable_raw(be, mr - 7, 8) == abi.RL_E_INVALID
        assert _enable_raw(be, 0xFFFFFFFF, 2) == abi.RL_E_INVALID
        assert be.L.rl_override_rules_info_get(be.ctx, C.byref(info)) == abi.RL_E_INVALID
        assert _enable_raw(be, mr - 8, 8) == abi.RL_OK  # (first_rule + capacity == max_rules)
        assert _enable_raw(be, nc, 8) == abi.RL_E_INVALID  # once per ctx
        got = be.override_rules_info()
        assert got == dict(first_rule=mr - 8, capacity=8, rules=0, key_bytes_used=0, key_bytes_cap=512, deferred_full=0)
        # a malformed message with an override before the malformation interns nothing
        bad = OC.message(b"c4", OC.desc(OC.entry(b"user", b"zz"), OC.limit(5, 1))) + bytes([0x12, 0x05, 0x0a])
        item = fl.submit_wire(be, [bad, ov_msg(b"user", b"u1"), ov_msg(b"user", b"u22")], [NOW] * 3, mr, 2)
        be.synchronize()
        assert item["wire"]["req_status"][:3].tolist() == [MALFORMED, OK, OK]
        assert be.override_rule_keys() == [b"c4.user_u1", b"c4.user_u22"] or \
            be.override_rule_keys() == [b"c4.user_u22", b"c4.user_u1"]
        rid = item["out"]["rule_id"][:2]
        assert sorted(rid.tolist()) == [mr - 8, mr - 7]
        # the sizing call and the range checks of rl_override_rule_keys
        need = C.c_uint64(0)
        off = np.zeros(3, np.uint32)
        L = be.L
        assert L.rl_override_rule_keys(be.ctx, mr - 8, 2, None, 0, abi.ptr(off), C.byref(need)) == abi.RL_E_CAPACITY
        assert need.value == 21 and off.tolist() in ([0, 10, 21], [0, 11, 21])
        buf = np.full(32, 0xEE, np.uint8)
        assert L.rl_override_rule_keys(be.ctx, mr - 8, 2, abi.ptr(buf), 20, abi.ptr(off), C.byref(need)) == abi.RL_E_CAPACITY
        assert (buf == 0xEE).all()
        assert L.rl_override_rule_keys(be.ctx, mr - 8, 2, abi.ptr(buf), 21, abi.ptr(off), None) == abi.RL_OK
        assert bytes(buf[:21]) in (b"c4.user_u1c4.user_u22", b"c4.user_u22c4.user_u1") and (buf[21:] == 0xEE).all()
        assert L.rl_override_rule_keys(be.ctx, mr - 7, 1, abi.ptr(buf), 32, abi.ptr(off), None) == abi.RL_OK
        assert L.rl_override_rule_keys(be.ctx, mr - 6, 0, None, 0, abi.ptr(off), None) == abi.RL_OK
        for frm, n in ((mr - 9, 1), (mr - 8, 3), (mr - 6, 1), (mr - 5, 0), (0, 1)):
            assert L.rl_override_rule_keys(be.ctx, frm, n, abi.ptr(buf), 32, abi.ptr(off), None) == abi.RL_E_INVALID
        with pytest.raises(RedisError):
            be.override_rule_keys(mr - 8, 3)
    finally:
        fl.close()
        be.close()
    # a multi-shard ctx, and one that joined a communicator
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=64, max_rules=16, n_shards=2)
    try:
        assert _enable_raw(be, 0, 8) == abi.RL_E_INVALID
    finally:
        be.close()
    be = Backend(0.8, False, table_slots=1 << 12, max_batch=64, max_rules=16)
    try:
        uid = loopback_id()
        be._check(be.L.rl_comm_init(be.ctx, 1, 0, abi.ptr(uid)))
        assert _enable_raw(be, 0, 8) == abi.RL_E_INVALID
    finally:
        be.close()
