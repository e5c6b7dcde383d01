"""GPU tests of the serialized responses (rl_do_limit_wire_respond_async,
rl_debug_respond; k_resp_size, k_resp_req, k_resp_emit, k_resp_to_host):
RateLimitResponse payloads written on the device. tests/response_ref.py, an
independent encoder held to the protobuf runtime by tests/test_respond_cpu.py,
is the reference for every byte.

1. rl_debug_respond on the edge list, at request counts around the tile, with
   a 300-descriptor request and a tile past the LDS budget;
2. responses at every byte alignment, guard bytes around the buffer;
3. the C4 request streams through should_rate_limit_responses_pipelined against
   the oracle service;
4. out, verdict and resp in one batch against the array path on a twin ctx;
5. deferred and malformed messages between good ones;
6. bytes_cap one below the bound fails its batch alone;
7. host-detected errors enqueue nothing;
8. wire, wire-respond and packed batches in flight keep submission order.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from oracle.config import OracleService, RateLimitConfig, StatsStore
from ratelimit_amd import abi
from ratelimit_amd.config import ConfigTree, pack_requests
from ratelimit_amd.limiter import Backend, GpuRateLimitService, PackedRequests, RedisError, WireRequests
from ratelimit_amd.packing import RuleInterner, pack_calls
import response_ref as R
import verdict_ref as V
import wire_cases as WC
from test_gpu_requests import FILES, SMALL, gen_requests, st_tuple
from test_gpu_requests_packed import GUARD, guards_intact, table_state
from test_gpu_verdict import STREAMS
from test_gpu_wire import Pair, WireFlight, cuts_of, encode, reference

pytestmark = pytest.mark.gpu

OK, DEFERRED, MALFORMED = abi.RL_WIRE_OK, abi.RL_WIRE_DEFERRED, abi.RL_WIRE_MALFORMED
STD_KEYS = R.KEY_SETS[3]
LONG_KEYS = R.KEY_SETS[4]


def split(raw, off):
    raw = bytes(raw)
    return [raw[int(off[q]):int(off[q + 1])] for q in range(len(off) - 1)]


def answers_of(reqs):
    req_idx, first, cols = R.arrays_of(reqs)
    return req_idx, first, {k: np.array(v, abi.REQUEST_RESULT_DTYPES[k]) for k, v in cols.items()}


@pytest.fixture(scope="module")
def backend():
    be = Backend(0.8, False, **SMALL)
    yield be
    be.close()


# ---- 1. the device serializer on explicit answers ---------------------------------------------

def debug_cases():
    """[(name, requests, header keys, global shadow)]"""
    edge = R.edge_requests()
    pool = edge + R.random_requests(3, 600)
    out = [("edge list", edge, STD_KEYS, False), ("edge list, shadow, no keys", edge, None, True),
           ("one empty request", [[]], STD_KEYS, False), ("300 descriptors alone", [edge[-1]], (b"", b"", b""), True)]
    for i, nq in enumerate((1, 255, 256, 257, 513)):
        out.append(("n=%d" % nq, pool[7 * i:7 * i + nq], R.KEY_SETS[i % len(R.KEY_SETS)], bool(i % 2)))
    # 256 one-descriptor requests with 64-byte keys: about 70 KB in one tile, past the LDS budget
    out.append(("a tile past the LDS budget", [[R.MAXIMAL]] * 256 + edge, LONG_KEYS, False))
    # only requests without descriptors: every head is the last tile's
    out.append(("no descriptors at all", [[]] * 300, STD_KEYS, False))
    # long runs of empty requests between descriptors, and at both ends
    out.append(("empty runs", [[]] * 270 + [[R.MAXIMAL] * 2] + [[]] * 300 + edge[:5] + [[]] * 260, LONG_KEYS, True))
    return out


@pytest.mark.parametrize("name,reqs,keys,gs", debug_cases(), ids=[c[0] for c in debug_cases()])
def test_gpu_debug_respond_equals_the_reference_encoder(backend, name, reqs, keys, gs):
    req_idx, first, ans = answers_of(reqs)
    raw, off = backend.debug_respond(len(reqs), req_idx, ans, keys, gs)
    want = [R.encode_request(d, gs, keys) for d in reqs]
    assert off[0] == 0 and int(off[-1]) == sum(map(len, want))
    got = split(raw[:int(off[-1])], off)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, q, reqs[q][:3])
    assert int(off[-1]) <= backend.response_bound(len(reqs), len(req_idx), keys)


def test_gpu_debug_respond_skips_refused_requests(backend):
    reqs = R.random_requests(4, 520)
    status = np.zeros(len(reqs), np.uint8)
    for q in list(range(0, len(reqs), 3)) + [len(reqs) - 1]:
        reqs[q] = []
        status[q] = 1 + q % 2
    req_idx, first, ans = answers_of(reqs)
    raw, off = backend.debug_respond(len(reqs), req_idx, ans, STD_KEYS, False, req_status=status)
    want = [b"" if status[q] else R.encode_request(d, False, STD_KEYS) for q, d in enumerate(reqs)]
    assert split(raw[:int(off[-1])], off) == want
    status[next(q for q, d in enumerate(reqs) if d)] = MALFORMED  # a refused request has no descriptors
    with pytest.raises(RedisError, match="RL_E_INVALID"):
        backend.debug_respond(len(reqs), req_idx, ans, STD_KEYS, False, req_status=status)


# ---- 2. alignments and guard bytes -----------------------------------------------------------

def test_gpu_debug_respond_alignments_and_guards(backend):
    seen_req, seen_tile = set(), set()
    for seed, keys in ((1, (b"a", b"bc", b"def")), (2, None), (3, STD_KEYS)):
        reqs = R.random_requests(40 + seed, 700)
        req_idx, first, ans = answers_of(reqs)
        want = [R.encode_request(d, False, keys) for d in reqs]
        cap = backend.response_bound(len(reqs), len(req_idx), keys)
        whole = np.full(cap + 64, GUARD, np.uint8)
        raw, off = backend.debug_respond(len(reqs), req_idx, ans, keys, False, bytes_cap=cap, out_bytes=whole[32:])
        total = int(off[-1])
        assert split(whole[32:32 + total], off) == want
        # nothing after resp_off[n], nothing around the buffer
        assert (whole[:32] == GUARD).all() and (whole[32 + total:] == GUARD).all() and total < cap
        seen_req |= {int(o) % 4 for o in off[:-1]}
        # where the tiles of 256 descriptors start (a status inside a request, or a request's head)
        for d0 in range(256, len(req_idx), 256):
            q = req_idx[d0]
            if first[q] == d0:
                seen_tile.add(int(off[q]) % 4)
            else:
                head = 2 + sum(len(R.encode_status(d)) for d in reqs[q][:d0 - first[q]])
                seen_tile.add((int(off[q]) + head) % 4)
    assert seen_req == {0, 1, 2, 3} and seen_tile == {0, 1, 2, 3}


# ---- 3. the streams against the oracle service ----------------------------------------------

def desc_of(st, unlimited):
    code, cl, rem, reset = st
    if cl is not None:
        return (code, R.LIMIT, cl[0], cl[1], rem, reset)
    return (code, R.UNLIMITED if unlimited else R.NONE, 0, 0, rem, 0)


@pytest.mark.parametrize("seed,keys", [(1, None), (1, STD_KEYS), (2, STD_KEYS)],
                         ids=["plain", "headers", "shadow+headers"])
def test_gpu_respond_stream_matches_oracle_service(seed, keys):
    p = STREAMS[seed]
    reqs, nows = gen_requests(seed, 1200)
    msgs = encode(reqs)
    cuts = cuts_of(seed, len(reqs))
    group = 12

    def deferred(q):  # a descriptor with a limit override
        return any(d.limit is not None for d in reqs[q].descriptors)

    order = []  # as the service applies them: per group the requests without an override, then the deferred ones
    for g in range(0, len(cuts), group):
        part = cuts[g:g + group]
        for i, j in part:
            order += [q for q in range(i, j) if not deferred(q)]
        for i, j in part:
            order += [q for q in range(i, j) if deferred(q)]
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
        want[q] = (v, [st_tuple(s) for s in osts], unl)
    ostats = {k: list(v.as_tuple()) for k, v in store.by_key.items() if any(v.as_tuple())}
    svc = GpuRateLimitService(FILES, 0.8, p["local_cache"], "", global_shadow_mode=p["global_shadow"],
                              header_keys=keys, **SMALL)
    got, shadow = [], 0
    try:
        for g in range(0, len(cuts), group):
            batches = [(msgs[i:j], nows[i:j]) for i, j in cuts[g:g + group]]
            for part, n in svc.should_rate_limit_responses_pipelined(batches):
                got += part
                shadow += n
        assert svc.global_shadow_count == shadow and len(got) == len(reqs)
        with_headers = over = 0
        for q, raw in enumerate(got):
            v, sts, unl = want[q]
            code, dsts, hdrs = R.decode_response(raw)
            assert code == v.code, q
            assert dsts == sts, q
            hw = [] if keys is None or v.headers is None else [(k, b"%d" % x) for k, x in zip(keys, v.headers)]
            assert hdrs == hw, q
            descs = [desc_of(s, u) for s, u in zip(sts, unl)]
            assert raw == R.encode_response(v.code, descs, v.headers, keys), q
            with_headers += bool(hdrs)
            over += v.flags & 1
        assert over > 0 and (with_headers > 200) == (keys is not None)
        assert dict(svc.stats) == ostats
        assert shadow == sum(v.shadow_inc for v, _, _ in want.values())
        assert (shadow > 0) == p["global_shadow"]
    finally:
        svc.close()


# ---- helpers for the raw entry point ----------------------------------------------------------

def submit_respond(fl, be, msgs, nows, n_rules, n_desc, keys, mode="both", global_shadow=False, bytes_cap=None):
    """A wire batch through rl_do_limit_wire_respond_async, every output guarded. n_desc: the descriptors the
    outputs hold; mode "none": neither out nor verdict."""
    s, buf, whole = fl.wire(msgs, nows, n_rules)
    nq = len(msgs)
    p = PackedRequests(s, buf, nq, n_desc, n_rules)
    out, ver, guards = (None, None, []) if mode == "none" else fl.outputs(p, mode)
    wire = {}
    for k, n, dt in (("req_status", nq, np.uint8), ("desc_first", nq + 1, np.uint32), ("n_descriptors", 1, np.uint32)):
        w, wire[k] = fl.guarded(n, dt)
        guards.append((w, wire[k]))
    cap = Backend.response_bound(nq, n_desc, keys) if bytes_cap is None else bytes_cap
    resp = {}
    w, resp["bytes"] = fl.guarded(cap, np.uint8)
    guards.append((w, resp["bytes"]))
    w, resp["resp_off"] = fl.guarded(nq + 1, np.uint32)
    guards.append((w, resp["resp_off"]))
    keep = be.do_limit_wire_respond_async(WireRequests(s, buf, nq, int(s.msgs_bytes)), wire, out, ver, resp, keys,
                                          global_shadow, n_desc, cap)
    item = dict(p=p, out=out, ver=ver, wire=wire, resp=resp, cap=cap, guards=guards + [(whole, buf)], keep=keep,
                packed=bytes(buf))
    fl.items.append(item)
    return item


def responses(item):
    nq = item["p"].n_requests
    off = item["resp"]["resp_off"][:nq + 1]
    total = int(off[nq])
    assert off[0] == 0 and total <= item["cap"]
    assert (item["resp"]["bytes"][total:item["cap"]] == GUARD).all()  # only the used bytes crossed
    return split(item["resp"]["bytes"][:total], off)


def host_responses(ref, st, keys):
    """rl_response_serialize over the arrays the array path returned."""
    nq = len(st)
    n = int(ref["wire"]["n_descriptors"][0])
    res = {k: ref["out"][k][:max(n, 1)] for k in abi.REQUEST_RESULT_DTYPES}
    ver = {k: ref["ver"][k][:nq] for k in abi.REQUEST_VERDICT_DTYPES}
    raw, off = Backend.response_serialize(ref["wire"]["desc_first"][:nq + 1], ref["wire"]["req_status"][:nq], res, ver,
                                          keys)
    return split(raw, off)


# ---- 4. against the array path ----------------------------------------------------------------

@pytest.mark.parametrize("mode", ["both", "none"])
def test_gpu_respond_equals_the_array_path(mode):
    reqs, nows = gen_requests(2, 700)
    msgs = encode(reqs)
    pr = Pair()
    try:
        flight = []
        for b, (i, j) in enumerate(cuts_of(5, len(reqs))):
            keys, gs = R.KEY_SETS[b % len(R.KEY_SETS)], bool(b % 2)
            st, a = reference(pr.pk, msgs[i:j], nows[i:j])
            n = len(a["req_idx"])
            ref = pr.fl.submit_wire(pr.ref_be, msgs[i:j], nows[i:j], pr.n_rules, n, "both", gs)
            item = submit_respond(pr.fl, pr.be, msgs[i:j], nows[i:j], pr.n_rules, n, keys, mode, gs)
            flight.append((item, ref, st, keys))
        pr.be.synchronize()
        pr.ref_be.synchronize()
        total = 0
        for item, ref, st, keys in flight:
            nq = len(st)
            n = int(ref["wire"]["n_descriptors"][0])
            assert item["wire"]["req_status"][:nq].tobytes() == st.tobytes() == ref["wire"]["req_status"][:nq].tobytes()
            assert item["wire"]["desc_first"][:nq + 1].tobytes() == ref["wire"]["desc_first"][:nq + 1].tobytes()
            if mode == "both":  # the arrays are those of rl_do_limit_wire_async
                for k in abi.REQUEST_RESULT_DTYPES:
                    assert item["out"][k][:n].tobytes() == ref["out"][k][:n].tobytes(), k
                for k in abi.REQUEST_VERDICT_DTYPES:
                    assert item["ver"][k][:nq].tobytes() == ref["ver"][k][:nq].tobytes(), k
                assert int(item["ver"]["global_shadow"][0]) == int(ref["ver"]["global_shadow"][0])
                assert host_responses(item, st, keys) == responses(item)
            got = responses(item)
            assert got == host_responses(ref, st, keys)
            assert [g == b"" for g in got] == list(st != OK)
            total += sum(map(len, got))
            guards_intact(item)
            guards_intact(ref)
        assert total > 10000
        assert table_state(pr.ref_be) == table_state(pr.be)
    finally:
        pr.close()


# ---- 5. deferred and malformed messages between good ones ---------------------------------------

def test_gpu_respond_bad_messages_between_good_ones():
    reqs, nows = gen_requests(5, 400)  # (with overrides: deferred messages)
    good = encode(reqs)
    bad = WC.malformed() + WC.truncations(good[:2]) + WC.flips(120, msgs=good)
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
            st, a = reference(pr.pk, msgs, ts)
            n = len(a["req_idx"])
            ref = pr.fl.submit_wire(pr.ref_be, msgs, ts, pr.n_rules, n)
            item = submit_respond(pr.fl, pr.be, msgs, ts, pr.n_rules, n, STD_KEYS, "none")
            flight.append((item, ref, st))
        pr.be.synchronize()
        pr.ref_be.synchronize()
        seen = np.zeros(3, np.int64)
        for item, ref, st in flight:
            got = responses(item)
            assert item["wire"]["req_status"][:len(st)].tobytes() == st.tobytes()
            assert [g == b"" for g in got] == list(st != OK)  # empty responses exactly where refused
            assert got == host_responses(ref, st, STD_KEYS)    # and unchanged neighbours
            for g in got:
                if g:
                    R.decode_response(g)
            seen += np.bincount(st, minlength=3)
            guards_intact(item)
        assert seen[MALFORMED] >= 50 and seen[DEFERRED] >= 3 and seen[OK] >= 100
        assert table_state(pr.ref_be) == table_state(pr.be)
    finally:
        pr.close()


# ---- 6. capacity, known once the device has counted -------------------------------------------

def test_gpu_respond_capacity_fails_at_synchronize():
    one = lambda i: O.Descriptor([("remote_address", "10.0.0.%d" % (i % 9))])  # noqa: E731
    mid = encode([O.RateLimitRequest("c4", [one(i), one(i + 1)], 1) for i in range(100)])  # 200 descriptors
    small, snow = gen_requests(9, 12, p_override=0.0)
    small = encode(small)
    n_small = sum(len(r.descriptors) for r in gen_requests(9, 12, p_override=0.0)[0])
    pr = Pair()
    try:
        bound = Backend.response_bound(100, 200, STD_KEYS)
        assert bound == 100 * (2 + 48 + sum(map(len, STD_KEYS))) + 26 * 200
        before = submit_respond(pr.fl, pr.be, small, snow, pr.n_rules, n_small, STD_KEYS)
        state = None
        bad = submit_respond(pr.fl, pr.be, mid, [1_700_000_040] * 100, pr.n_rules, 200, STD_KEYS, bytes_cap=bound - 1)
        with pytest.raises(RedisError, match="RL_E_CAPACITY"):
            pr.be.synchronize()
        state = table_state(pr.be)
        assert (bad["resp"]["bytes"] == GUARD).all()
        guards_intact(bad)
        # the table has seen the first batch alone: the twin after that batch is in the same state
        ref = pr.fl.submit_wire(pr.ref_be, small, snow, pr.n_rules, n_small)
        pr.ref_be.synchronize()
        assert table_state(pr.ref_be) == state
        st = np.zeros(len(small), np.uint8)
        assert responses(before) == host_responses(ref, st, STD_KEYS)
        # the next batch answers normally; so does the refused one with the bound's capacity
        after = submit_respond(pr.fl, pr.be, mid, [1_700_000_040] * 100, pr.n_rules, 200, STD_KEYS, bytes_cap=bound)
        pr.be.synchronize()
        ref = pr.fl.submit_wire(pr.ref_be, mid, [1_700_000_040] * 100, pr.n_rules, 200)
        pr.ref_be.synchronize()
        assert responses(after) == host_responses(ref, np.zeros(100, np.uint8), STD_KEYS)
        assert table_state(pr.ref_be) == table_state(pr.be)
    finally:
        pr.close()


# ---- 7. host-detected errors -----------------------------------------------------------------

def test_gpu_respond_host_detected_errors_enqueue_nothing():
    it = RuleInterner()
    tree = ConfigTree.from_yaml(FILES, "", it)
    be = Backend(0.8, True, **SMALL)
    two = Backend(0.8, True, n_shards=2, shard_devices=[0, 0], hash_seed=5, **SMALL)
    fl = WireFlight()
    try:
        for b in (be, two):
            b.load_config(tree)
        reqs, nows = gen_requests(41, 300, p_override=0.0)
        msgs = encode(reqs)
        n = sum(len(r.descriptors) for r in reqs)
        s, buf, whole = fl.wire(msgs, nows, len(it.keys))
        nq = len(msgs)
        cap = Backend.response_bound(nq, n, STD_KEYS)
        w_status, status = fl.guarded(nq, np.uint8)
        w_bytes, rbytes = fl.guarded(cap, np.uint8)
        w_off, roff = fl.guarded(nq + 1, np.uint32)
        pageable = np.zeros(cap, np.uint8)
        fill = [bytes(w.view(np.uint8)) for w in (w_status, w_bytes, w_off)]

        def call(b, keys=STD_KEYS, resp=True, rb=rbytes, ro=roff, reserved=0, null_key=False, cap=cap):
            wr = abi.RlWireResult()
            wr.req_status = abi.ptr(status)
            wr.desc_cap = n
            f, keep = abi.make_response_format(keys)
            f.reserved = reserved
            if null_key:
                f.remaining_key = None
            r = abi.RlResponseBatch()
            r.bytes, r.bytes_cap, r.resp_off = abi.ptr(rb), cap, abi.ptr(ro)
            return b.L.rl_do_limit_wire_respond_async(b.ctx, C.byref(s), C.byref(wr), None, 0, None, C.byref(f),
                                                      C.byref(r) if resp else None)

        sub0 = be.batch_progress()[0]
        assert call(be, resp=False) == abi.RL_E_INVALID                      # no rl_response_batch
        assert call(be, rb=None) == abi.RL_E_INVALID                         # null bytes
        assert call(be, ro=None) == abi.RL_E_INVALID                         # null resp_off
        assert call(be, keys=(b"k" * 65, b"", b"")) == abi.RL_E_INVALID      # a key over 64 bytes
        assert call(be, null_key=True) == abi.RL_E_INVALID                   # a NULL key with a length
        assert call(be, reserved=1) == abi.RL_E_INVALID
        assert call(be, rb=pageable) == abi.RL_E_INVALID                     # pageable memory
        assert b"page-locked" in be.L.rl_last_error(be.ctx)
        assert call(be, cap=cap + (1 << 34)) == abi.RL_E_INVALID             # bytes_cap past the allocation
        assert call(two) == abi.RL_E_INVALID                                 # single-shard ctxs only
        assert be.batch_progress()[0] == sub0
        assert fill == [bytes(w.view(np.uint8)) for w in (w_status, w_bytes, w_off)]
        assert be.table_info()["decisions"] == 0 and be.table_info()["live_slots"] == 0
        # the good call goes through, out and verdict both NULL
        assert call(be) == abi.RL_OK
        assert be.batch_progress()[0] == sub0 + 1
        be.synchronize()
        assert be.table_info()["decisions"] > 0 and (status == OK).all()
        assert roff[0] == 0 and 2 * nq < int(roff[nq]) <= cap
        for g in split(rbytes[:int(roff[nq])], roff):
            assert R.decode_response(g)[0] in (1, 2)
        assert bytes(buf) == bytes(fl.wire(msgs, nows, len(it.keys))[1])    # the batch's buffer is only read
    finally:
        fl.close()
        for b in (be, two):
            b.close()


# ---- 8. order ----------------------------------------------------------------------------------

def test_gpu_respond_interleaves_in_submission_order():
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
        first = submit_respond(fl, be, msgs, [now] * 20, len(it.keys), 20, STD_KEYS, "none")
        second = fl.submit_wire(be, msgs, [now] * 20, len(it.keys), 20)     # the array path
        third = fl.submit(be, a, len(it.keys))                              # the packed path
        mid = be.do_limit_packed(pb)                                        # rl_do_limit on the same keys
        fourth = submit_respond(fl, be, msgs, [now] * 20, len(it.keys), 20, None, "both")
        be.synchronize()
        h = np.array([1 + i % 3 for i in range(len(tenants))])

        def remaining(item):
            out = []
            for g in responses(item):
                code, sts, hdrs = R.decode_response(g)
                assert code == 1 and len(sts) == 1 and sts[0][1] == (40, O.HOUR)
                out.append(sts[0][2])
            return out

        assert remaining(first) == list(40 - h)
        assert list(second["out"]["limit_remaining"][:20]) == list(40 - 2 * h)
        assert list(third["out"]["limit_remaining"][:20]) == list(40 - 3 * h)
        assert list(mid["limit_remaining"]) == list(40 - 3 * h - 5)
        assert remaining(fourth) == list(40 - 4 * h - 5) == list(fourth["out"]["limit_remaining"][:20])
        # the first batch's headers carry its descriptor's values
        code, sts, hdrs = R.decode_response(responses(first)[0])
        assert hdrs == [(STD_KEYS[0], b"40"), (STD_KEYS[1], b"%d" % (40 - h[0])), (STD_KEYS[2], b"%d" % sts[0][3])]
    finally:
        fl.close()
        be.close()
