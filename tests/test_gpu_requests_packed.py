"""GPU tests of the pipelined request path (rl_do_limit_requests_packed_async,
k_unpack_requests): one-buffer request batches answered without waiting.

1. the C4 request streams of tests/test_gpu_verdict.py through
   should_rate_limit_verdicts_pipelined, 3 x RL_REQUESTS_INFLIGHT batches per
   rl_synchronize, against the oracle service;
2. bytewise equality with rl_do_limit_requests_verdict in every output mode;
3. the shapes at the unpack kernel's edges, one by one and all in flight;
4. batches malformed on the device: RL_E_INVALID at rl_synchronize, the table
   and the neighbouring batches untouched, no write outside the outputs;
5. host-detected errors: refused at the call, nothing enqueued;
6. interleaving with rl_do_limit and rl_lookup keeps submission order;
7. rl_batch_progress alone completes the batches in flight.
"""
import ctypes as C
import random
import time

import numpy as np
import pytest

from oracle import oracle as O
from ratelimit_amd import abi
from ratelimit_amd.config import ConfigTree, pack_requests
from ratelimit_amd.limiter import Backend, GpuRateLimitService, PackedRequests, PinnedArena, RedisError
from ratelimit_amd.packing import RuleInterner, pack_calls
from test_gpu_requests import FILES, SMALL, gen_requests
from test_gpu_verdict import STREAMS, check_against_oracle, oracle_stream

pytestmark = pytest.mark.gpu

INFLIGHT = abi.RL_REQUESTS_INFLIGHT
TILE = abi.RL_REQUESTS_TILE
DIVIDER = {O.SECOND: 1, O.MINUTE: 60, O.HOUR: 3600, O.DAY: 86400}
GUARD = 0x5A


def slices(seed, n):
    """The random slices {1, 7, 64, 300} of test_gpu_verdict.run_stream."""
    rng = random.Random(seed * 7)
    cuts, i = [], 0
    while i < n:
        j = min(n, i + rng.choice([1, 7, 64, 300]))
        cuts.append((i, j))
        i = j
    return cuts


# ---- 1. stream parity while in flight -----------------------------------------------

@pytest.mark.parametrize("seed", [1, 2])
def test_gpu_packed_stream_matches_oracle_service(seed):
    reqs, nows, verdicts, statuses, _ = oracle_stream(seed)
    cuts = slices(seed, len(reqs))
    # (CPU, from the oracle's run) descriptors that hit a (key, window) the batch submitted just before
    # them also hit: a second half enqueued out of order would answer these differently
    def keys(i, j):
        out = []
        for r, now, sts in zip(reqs[i:j], nows[i:j], statuses[i:j]):
            for d, s in zip(r.descriptors, sts):
                if s[1] is not None:  # a limited descriptor: it reached DoLimit
                    out.append((r.domain, tuple(d.entries), now // DIVIDER[s[1][1]], s[1][1]))
        return out

    per_batch = [keys(i, j) for i, j in cuts]
    chained = sum(sum(1 for k in cur if k in prev) for prev, cur in zip(map(set, per_batch), per_batch[1:]))
    assert chained >= 100, chained
    p = STREAMS[seed]
    svc = GpuRateLimitService(FILES, 0.8, p["local_cache"], "", global_shadow_mode=p["global_shadow"], **SMALL)
    got, shadow = [], 0
    try:
        group = 3 * INFLIGHT
        for g in range(0, len(cuts), group):
            batches = [(reqs[i:j], nows[i:j]) for i, j in cuts[g:g + group]]
            for part, n in svc.should_rate_limit_verdicts_pipelined(batches):
                got += part
                shadow += n
        assert svc.global_shadow_count == shadow
        check_against_oracle(seed, got, dict(svc.stats), shadow)
    finally:
        svc.close()


# ---- helpers for the raw entry point ----------------------------------------------------

class Flight:
    """Packed batches and their guarded pinned outputs, kept alive until read."""

    def __init__(self):
        self.arena = PinnedArena()
        self.items = []

    def guarded(self, n, dtype):
        """A pinned array with 16 guard bytes before and after it -> (whole, view)."""
        dt = np.dtype(dtype)
        pad = 16 // dt.itemsize
        whole = self.arena.array(n + 2 * pad, dt)
        whole.view(np.uint8)[:] = GUARD
        return whole, whole[pad:pad + n]

    def pack(self, be, a, n_rules):
        """rl_request_batch_pack into a guarded pinned buffer."""
        probe = be.pack_requests(a, n_rules)  # (pageable: the size and the struct)
        size = int(probe.struct.buf_bytes)
        whole, buf = self.guarded(size, np.uint8)
        buf[:] = probe.buf[:size]
        s = abi.RlRequestBatchPacked.from_buffer_copy(probe.struct)
        s.buf = buf.ctypes.data
        self.items.append(whole)
        return PackedRequests(s, buf, probe.n_requests, probe.n_descriptors, n_rules), whole

    def outputs(self, p, mode):
        """mode: "out", "verdict" or "both" -> (out dict or None, verdict dict or None, guards)."""
        out = ver = None
        guards = []
        if mode in ("out", "both"):
            out = {}
            for k, dt in abi.REQUEST_RESULT_DTYPES.items():
                w, out[k] = self.guarded(p.n_descriptors, dt)
                guards.append((w, out[k]))
            w, out["stats"] = self.guarded(p.n_rules * abi.RL_NUM_STATS, np.uint64)
            guards.append((w, out["stats"]))
        if mode in ("verdict", "both"):
            ver = {}
            for k, dt in abi.REQUEST_VERDICT_DTYPES.items():
                w, ver[k] = self.guarded(p.n_requests, dt)
                guards.append((w, ver[k]))
            w, ver["global_shadow"] = self.guarded(1, np.uint64)
            guards.append((w, ver["global_shadow"]))
        return out, ver, guards

    def submit(self, be, a, n_rules, mode="both", global_shadow=False):
        p, whole = self.pack(be, a, n_rules)
        out, ver, guards = self.outputs(p, mode)
        keep = be.do_limit_requests_packed_async(p, out, ver, global_shadow)
        item = dict(p=p, out=out, ver=ver, guards=guards + [(whole, p.buf)], keep=keep, packed=bytes(p.buf))
        self.items.append(item)
        return item

    def close(self):
        self.arena.close()


def guards_intact(item):
    for whole, view in item["guards"]:
        w8, pad = whole.view(np.uint8), 16
        n8 = view.size * view.dtype.itemsize
        assert (w8[:pad] == GUARD).all() and (w8[pad + n8:pad + n8 + pad] == GUARD).all()
    assert bytes(item["p"].buf) == item["packed"]  # the batch's own buffer is only read


def sync_reference(be, a, n_rules, mode="both", global_shadow=False):
    """The same batch through rl_do_limit_requests_verdict."""
    return be.do_limit_requests_verdict(a, n_rules, global_shadow, per_descriptor=mode != "verdict",
                                        stats=mode != "verdict")


def assert_same(item, ref, mode="both"):
    n, nq, nr = item["p"].n_descriptors, item["p"].n_requests, item["p"].n_rules
    if mode in ("out", "both"):
        for k in abi.REQUEST_RESULT_DTYPES:
            assert item["out"][k][:n].tobytes() == ref[k].tobytes(), k
        assert item["out"]["stats"][:nr * abi.RL_NUM_STATS].tobytes() == ref["stats"].tobytes()
    if mode in ("verdict", "both"):
        for k in abi.REQUEST_VERDICT_DTYPES:
            assert item["ver"][k][:nq].tobytes() == ref[k].tobytes(), k
        assert int(item["ver"]["global_shadow"][0]) == ref["global_shadow"]
    guards_intact(item)


def table_state(be, now=1_700_000_050):
    t = be.table_info()
    return {k: t[k] for k in ("live_slots", "batches", "decisions")}, be.local_cache_info(now)


def backend_pair(**kw):
    it = RuleInterner()
    tree = ConfigTree.from_yaml(FILES, "", it)
    cfg = dict(SMALL, hash_seed=77)
    cfg.update(kw)
    bes = [Backend(0.8, True, **cfg) for _ in range(2)]
    for be in bes:
        be.load_config(tree)
    return bes, it


# ---- 2. bytewise equality with the synchronous path --------------------------------------

def test_gpu_packed_equals_the_sync_path_bytewise():
    reqs, nows = gen_requests(2, 600)
    (sync_be, async_be), it = backend_pair()
    fl = Flight()
    try:
        cuts = slices(3, len(reqs))
        modes = ["out", "verdict", "both"]
        for g in range(0, len(cuts), 2 * INFLIGHT + 1):
            flight = []
            for b, (i, j) in enumerate(cuts[g:g + 2 * INFLIGHT + 1]):
                a = pack_requests(reqs[i:j], nows[i:j], it)
                mode = modes[(g + b) % 3]
                flight.append((fl.submit(async_be, a, len(it.keys), mode, True),
                               sync_reference(sync_be, a, len(it.keys), "both" if mode == "out" else mode, True), mode))
            async_be.synchronize()
            for item, ref, mode in flight:
                assert_same(item, ref, mode)
        assert table_state(sync_be) == table_state(async_be)
    finally:
        fl.close()
        sync_be.close()
        async_be.close()


# ---- 3. the shapes at the kernel's edges ---------------------------------------------------

def edge_batches():
    """[(name, requests, nows)] in the c4 / test-domain config of the request tests."""
    rng = random.Random(5)
    out = []
    for nq in (0, 1, 255, 256, 257, 513):
        out.append(("n_requests=%d" % nq,) + gen_requests(100 + nq, nq))

    def one(i):
        return O.Descriptor([("remote_address", "10.0.0.%d" % (i % 7))])

    def req(descs, dom="c4"):
        return O.RateLimitRequest(dom, descs, rng.randint(1, 3))

    # a request of 300 descriptors that starts at descriptor 100: it straddles the tile's first 256-descriptor chunk
    rs = [req([one(i)]) for i in range(100)] + [req([one(i) for i in range(300)])] + [req([one(i)]) for i in range(200)]
    out.append(("300 descriptors across a chunk", rs, [1_700_000_041] * len(rs)))
    # requests without descriptors at a tile's start and end (tiles 0 and 1)
    rs = [req([] if i in (0, 255, 256, 511) else [one(i), one(i + 1)]) for i in range(600)]
    out.append(("empty requests at tile ends", rs, [1_700_000_041] * len(rs)))
    # descriptors without entries
    rs = [req([O.Descriptor([]), one(i), O.Descriptor([])]) for i in range(40)] + [req([O.Descriptor([])])]
    out.append(("descriptors without entries", rs, [1_700_000_042] * len(rs)))
    # entries long enough for k_match's global-memory fallback (test_gpu_requests' lengths)
    vals = ["v" + "x_" * rng.randint(40, 150) + str(i) for i in range(40)]
    rs = [req([O.Descriptor([("tenant", rng.choice(vals))]), O.Descriptor([("tenant", rng.choice(vals)), ("tier", "x_y")]),
               O.Descriptor([("remote_address", rng.choice(vals))])]) for _ in range(300)]
    out.append(("long entries", rs, [1_700_000_042] * len(rs)))
    out.append(("ordinary before",) + gen_requests(31, 90))
    rs = [req([one(i), one(i + 3)], "nope") for i in range(300)]  # unknown domains only: nothing matches
    out.append(("unknown domains only", rs, [1_700_000_042] * len(rs)))
    out.append(("ordinary after",) + gen_requests(32, 90))
    # overrides on the first and the last descriptor of a tile (requests 256 and 511 of 600, two descriptors each)
    rs = []
    for i in range(600):
        d = [one(i), one(i + 1)]
        if i == 256:
            d[0] = O.Descriptor(d[0].entries, O.Limit(3, O.MINUTE))
        if i == 511:
            d[1] = O.Descriptor(d[1].entries, O.Limit(2, O.HOUR))
        if i == 0:
            d[0] = O.Descriptor(d[0].entries, O.Limit(1, O.SECOND))
        rs.append(req(d))
    out.append(("overrides at tile ends", rs, [1_700_000_043] * len(rs)))
    rs = [req([one(i)]) for i in range(30)]  # no overrides: a zero-length section
    out.append(("no overrides", rs, [1_700_000_043] * len(rs)))
    return out


@pytest.mark.parametrize("together", [False, True], ids=["one by one", "all in flight"])
def test_gpu_packed_edge_shapes_equal_the_sync_path(together):
    (sync_be, async_be), it = backend_pair(max_stem_bytes=1 << 22)
    fl = Flight()
    try:
        flight = []
        for name, rs, nows in edge_batches():
            a = pack_requests(rs, nows, it)
            item = fl.submit(async_be, a, len(it.keys))
            if name == "no overrides":
                assert item["p"].struct.n_overrides == 0
            if name == "overrides at tile ends":
                assert item["p"].struct.n_overrides == 3
            ref = sync_reference(sync_be, a, len(it.keys))
            if name == "unknown domains only":
                assert not ref["match"].any()
            if not together:
                async_be.synchronize()
                assert_same(item, ref)
            flight.append((name, item, ref))
        async_be.synchronize()
        for name, item, ref in flight:
            assert_same(item, ref)
        assert table_state(sync_be) == table_state(async_be)
    finally:
        fl.close()
        sync_be.close()
        async_be.close()


# ---- 4. malformed on the device -------------------------------------------------------------

def corrupt(p, case):
    """Damage the packed buffer in place (the struct's sizes stay as they are)."""
    s, buf = p.struct, p.buf
    if case.startswith("index"):
        ix = buf[s.index:s.index + 16 * 3].view(np.uint32)
        ix[4 + int(case[-1])] += 1  # entry 1, one component
        return
    ov = buf[s.overrides:s.overrides + 16 * s.n_overrides]
    w = ov.view(np.uint32)
    if case == "override index == n_descriptors":
        w[4 * (s.n_overrides - 1)] = s.n_descriptors
    elif case == "override list not increasing":
        w[4] = w[0]
    elif case == "override reserved byte":
        ov[16 + 14] = 1
    else:
        raise AssertionError(case)


MALFORMED = ["index 0", "index 1", "index 2", "index 3", "override index == n_descriptors",
             "override list not increasing", "override reserved byte"]


def test_gpu_packed_malformed_batches_fail_alone():
    (ref_be, be), it = backend_pair()
    fl = Flight()
    try:
        rng = random.Random(9)
        for k, case in enumerate(MALFORMED):
            ra, na = gen_requests(200 + k, 120)
            rc_, nc = gen_requests(300 + k, 120)
            rb = []
            for i in range(400):  # two tiles, a few overrides
                d = [O.Descriptor([("remote_address", "10.0.0.%d" % rng.randrange(9))]) for _ in range(2)]
                if i % 100 == 7:
                    d[1] = O.Descriptor(d[1].entries, O.Limit(4, O.MINUTE))
                rb.append(O.RateLimitRequest("c4", d, 1))
            aa, ab, ac = (pack_requests(ra, na, it), pack_requests(rb, [1_700_000_043] * 400, it),
                          pack_requests(rc_, nc, it))
            n_rules = len(it.keys)
            before = fl.submit(be, aa, n_rules)
            # the bad batch: packed, then damaged, then submitted (the host checks pass)
            p, whole = fl.pack(be, ab, n_rules)
            assert p.struct.n_overrides == 4 and p.n_requests > TILE
            corrupt(p, case)
            out, ver, guards = fl.outputs(p, "both")
            keep = be.do_limit_requests_packed_async(p, out, ver, False)
            bad = dict(p=p, out=out, ver=ver, guards=guards + [(whole, p.buf)], keep=keep, packed=bytes(p.buf))
            after = fl.submit(be, ac, n_rules)
            with pytest.raises(RedisError, match="RL_E_INVALID"):
                be.synchronize()
            be.synchronize()  # reported once
            assert_same(before, sync_reference(ref_be, aa, n_rules))
            assert_same(after, sync_reference(ref_be, ac, n_rules))
            guards_intact(bad)
            assert table_state(ref_be) == table_state(be), case  # the bad batch never ran
    finally:
        fl.close()
        ref_be.close()
        be.close()


# ---- 5. host-detected errors ----------------------------------------------------------------------

def test_gpu_packed_host_detected_errors_enqueue_nothing():
    it = RuleInterner()
    tree = ConfigTree.from_yaml(FILES, "", it)
    be = Backend(0.8, True, **SMALL)
    small = Backend(0.8, True, max_stem_bytes=64, **SMALL)
    bare = Backend(0.8, True, **SMALL)
    two = Backend(0.8, True, n_shards=2, shard_devices=[0, 0], hash_seed=5, **SMALL)
    fl = Flight()
    try:
        for b in (be, small, two):
            b.load_config(tree)
        reqs, nows = gen_requests(41, 300)
        a = pack_requests(reqs, nows, it)
        n_rules = len(it.keys)
        p, _ = fl.pack(be, a, n_rules)
        out, ver, _ = fl.outputs(p, "both")

        def call(b, s, out=out, ver=ver, opts=0):
            r = v = None
            if out is not None:
                r = abi.RlRequestResult()
                for k in out:
                    setattr(r, k, abi.ptr(out[k]))
            if ver is not None:
                v = abi.RlRequestVerdict()
                for k in ver:
                    setattr(v, k, abi.ptr(ver[k]))
            return b.L.rl_do_limit_requests_packed_async(b.ctx, C.byref(s), C.byref(r) if r else None, opts,
                                                         C.byref(v) if v else None)

        def changed(**fields):
            s = abi.RlRequestBatchPacked.from_buffer_copy(p.struct)
            for k, x in fields.items():
                setattr(s, k, x)
            return s

        B = int(p.struct.buf_bytes)
        sub0 = be.batch_progress()[0]
        sections = ("req", "now", "hits", "desc", "key_len", "value_len", "domain_bytes", "entry_bytes", "overrides",
                    "index")
        for k in sections:
            assert call(be, changed(**{k: B + 4})) == abi.RL_E_INVALID, k       # outside buf
            assert call(be, changed(**{k: getattr(p.struct, k) + 2})) == abi.RL_E_INVALID, k  # not 4-byte aligned
        assert call(be, changed(buf_bytes=B - 4)) == abi.RL_E_INVALID            # the last section cut short
        assert call(be, changed(n_descriptors=SMALL["max_batch"] + 1)) == abi.RL_E_CAPACITY
        assert call(be, changed(n_requests=SMALL["max_batch"] + 1)) == abi.RL_E_CAPACITY
        assert call(be, changed(n_rules=SMALL["max_rules"] + 1)) == abi.RL_E_CAPACITY
        assert call(be, changed(n_descriptors=p.n_descriptors - 1)) == abi.RL_E_INVALID  # the index's totals
        assert call(be, changed(), opts=2) == abi.RL_E_INVALID                  # unknown opts bit
        assert call(be, changed(), out=None, ver=None) == abi.RL_E_INVALID      # both outputs NULL
        assert be.batch_progress()[0] == sub0
        sub0 = small.batch_progress()[0]
        assert call(small, changed()) == abi.RL_E_CAPACITY                      # entry bytes over max_stem_bytes
        assert small.batch_progress()[0] == sub0
        sub0 = bare.batch_progress()[0]
        assert call(bare, changed()) == abi.RL_E_INVALID                        # no config loaded
        assert b"configuration" in bare.L.rl_last_error(bare.ctx)
        assert bare.batch_progress()[0] == sub0
        assert call(two, changed()) == abi.RL_E_INVALID                         # single-shard ctxs only
        assert b"rl_do_limit_requests_verdict" in two.L.rl_last_error(two.ctx)
        # nothing ran: the table is empty, and the good batch still goes through
        assert be.table_info()["decisions"] == 0 and be.table_info()["live_slots"] == 0
        sub0 = be.batch_progress()[0]
        assert call(be, changed()) == abi.RL_OK
        assert be.batch_progress()[0] == sub0 + 1
        be.synchronize()
        assert be.table_info()["decisions"] > 0
    finally:
        fl.close()
        for b in (be, small, bare, two):
            b.close()


# ---- 6. interleaving ----------------------------------------------------------------------------------

def test_gpu_packed_interleaves_in_submission_order():
    it = RuleInterner()
    tree = ConfigTree.from_yaml(FILES, "", it)
    be = Backend(0.8, False, **SMALL)
    fl = Flight()
    try:
        be.load_config(tree)
        now = 1_700_003_000
        tenants = ["t%d" % i for i in range(20)]
        reqs = [O.RateLimitRequest("c4", [O.Descriptor([("tenant", t)])], 1 + i % 3) for i, t in enumerate(tenants)]
        a = pack_requests(reqs, [now] * len(reqs), it)
        lim = O.new_rate_limit(40, O.HOUR, "c4.tenant")
        pb = pack_calls([(O.RateLimitRequest("c4", [O.Descriptor([("tenant", t)])], 5), [lim], now) for t in tenants],
                        "", RuleInterner())
        first = fl.submit(be, a, len(it.keys))
        mid = be.do_limit_packed(pb)                  # rl_do_limit on the same keys
        second = fl.submit(be, a, len(it.keys))
        off = pb.arrays["stem_off"]
        stems = [bytes(pb.arrays["stem_bytes"][off[i]:off[i + 1]]) for i in range(len(tenants))]
        look = be.lookup(stems, [O.HOUR] * len(stems), [now] * len(stems))  # completes the pending batch first
        h = np.array([1 + i % 3 for i in range(len(tenants))])
        assert list(mid["limit_remaining"]) == list(40 - h - 5)
        assert list(look["count"]) == list(2 * h + 5) and look["found"].all()
        be.synchronize()  # (the asynchronous outputs are read after it)
        assert list(first["out"]["limit_remaining"][:20]) == list(40 - h)
        assert list(second["out"]["limit_remaining"][:20]) == list(40 - 2 * h - 5)
        assert (first["out"]["match"][:20] == abi.RL_MATCH_LIMIT).all()
    finally:
        fl.close()
        be.close()


# ---- 7. progress without another submit ----------------------------------------------------------------

def test_gpu_packed_progress_completes_the_flight():
    (sync_be, be), it = backend_pair()
    fl = Flight()
    try:
        flight = []
        for k in range(INFLIGHT):
            reqs, nows = gen_requests(50 + k, 200)
            a = pack_requests(reqs, nows, it)
            flight.append((fl.submit(be, a, len(it.keys)), sync_reference(sync_be, a, len(it.keys))))
        deadline = time.monotonic() + 10
        while True:
            sub, done = be.batch_progress()
            assert sub == INFLIGHT
            if done == sub:
                break
            assert time.monotonic() < deadline, (sub, done)
            time.sleep(0.001)
        for item, ref in flight:  # (no rl_synchronize so far)
            assert_same(item, ref)
        be.synchronize()
        assert table_state(sync_be) == table_state(be)
    finally:
        fl.close()
        sync_be.close()
        be.close()
