"""Request-path throughput (rl_do_limit_requests): C1 / C2 batches as raw
requests (domain + entry bytes), matched against the C1 config on the GPU
(GetLimit trie walk), compacted into DoLimit and mapped back.

Host buffers (pinned, rl_alloc_host), synchronous: the number is PCIe-inclusive
(raw request bytes in, per-descriptor results out) and includes the one
mid-call count readback. The same batches through the packed DoLimit path
(rl_do_limit, also host buffers) are timed beside it, and both results are
checked equal (the request path must give DoLimit's answers).

--verdict full adds the per-request verdict (rl_do_limit_requests_verdict:
overall code, header values, global shadow mode); --verdict only also drops
the per-descriptor outputs (out == NULL), so that only per-request bytes come
back. off (the default) is rl_do_limit_requests as before.

--path packed-async takes the same batches through the pipelined entry point
(rl_do_limit_requests_packed_async): each batch converted once into the
one-buffer layout (rl_request_batch_pack), --steps batches submitted back to
back with one rl_synchronize at the end, under the same --verdict modes. A
buffer and its outputs are reused only once rl_batch_progress counts their
previous batch complete (a ring of PACKED_RING buffers), as a batcher would.

--path wire-async submits the same batches as serialized RateLimitRequest
payloads (rl_do_limit_wire_async: parsed on the GPU), from a ring of
PACKED_RING pinned buffers in the same way.

--from-payloads starts both pipelined paths from the same C1 payload bytes in
pageable memory, inside the timed loop: packed-async runs rl_packer_pack +
rl_request_batch_pack on each batch's messages, split over --pack-threads N
(<= 16) host threads, each slice submitted as its own packed batch; wire-async
copies the payload bytes into its pinned buffer and writes the offsets and
clocks.

--respond (with --path wire-async) takes the answers back as serialized
RateLimitResponse payloads written on the GPU (rl_do_limit_wire_respond_async)
instead of the per-descriptor and per-request arrays: out carries the stats
alone and verdict is NULL in the timed loop. The warm-up batches return both
and check the device's bytes against rl_response_serialize over the arrays;
that host step is then timed on 1, 4 and 16 threads (one contiguous slice of
the requests per thread): it is what the device spares the host.
--respond-headers is --respond with the three RateLimit-* header names
configured, so that every response also carries its three HeaderValues.

--override-share P (with --path wire-async --from-payloads) gives a share P of
the requests a ``limit`` override on their first descriptor (requests_per_unit
1000, SECOND); their tenants are folded onto OVERRIDE_TENANTS values, so the
set of override stats keys is small and stable, as a fleet's per-route
overrides are. Without --device-overrides the device defers those messages and
the host answers them as a service does today: when a buffer's batch is
complete, its deferred messages go through rl_packer_pack and the synchronous
rl_do_limit_requests, inside the timed loop. With --device-overrides the ctx
interns the override stats keys on the GPU (rl_override_rules_enable) and the
timed loop is the plain wire loop; the warm-up checks that nothing is deferred.
The rate counts every descriptor of every request either way. The parity check
against the packed DoLimit path is skipped (the overrides change the limits).

    python scripts/bench_requests.py [--config c1|c2] [--steps K] [--verdict off|full|only]
                                     [--path sync|packed-async|wire-async] [--respond | --respond-headers]
                                     [--from-payloads [--pack-threads N]]
                                     [--override-share P [--device-overrides]]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ratelimit_amd import abi, workloads as W  # noqa: E402
from ratelimit_amd._lib import lib  # noqa: E402
from ratelimit_amd.config import ConfigTree  # noqa: E402
from ratelimit_amd.limiter import Backend, PinnedArena  # noqa: E402

PACKED_RING = 8  # packed buffers (and output sets) in rotation on --path packed-async
HEADER_KEYS = (b"RateLimit-Limit", b"RateLimit-Remaining", b"RateLimit-Reset")  # --respond-headers
OVERRIDE_TENANTS = 1024   # --override-share: distinct tenants (override stats keys) among the override requests
OVERRIDE_CAPACITY = 4096  # --device-overrides: rl_override_rules_config.capacity
OVERRIDE_LIMIT = bytes([0x12, 0x05, 0x08, 0xE8, 0x07, 0x10, 0x01])  # limit {requests_per_unit: 1000, unit: SECOND}


def override_payloads(rows, tenants, share, rng):
    """c1_payloads' rows with a share of the requests carrying OVERRIDE_LIMIT on their first descriptor
    -> (the payload bytes, uint32 offsets [nq + 1], the override requests' indices)."""
    nq, L = rows.shape
    mask = rng.random(nq) < share
    idx = np.nonzero(mask)[0]
    ov = W.c1_payloads(np.asarray(tenants)[idx] % OVERRIDE_TENANTS, rows[idx, -1])
    d0 = 2 + rows[0, 1]  # the first descriptor: tag, length, body (after the domain field)
    assert rows[0, d0] == 0x12 and rows[0, d0 + 1] + len(OVERRIDE_LIMIT) < 128
    end = d0 + 2 + rows[0, d0 + 1]
    lim = np.tile(np.frombuffer(OVERRIDE_LIMIT, np.uint8), (len(idx), 1))
    ov = np.concatenate([ov[:, :end], lim, ov[:, end:]], axis=1)
    ov[:, d0 + 1] += len(OVERRIDE_LIMIT)
    lens = np.where(mask, ov.shape[1], L).astype(np.uint64)
    off = np.zeros(nq + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = np.empty(int(off[-1]), np.uint8)
    plain = np.nonzero(~mask)[0]
    flat[(off[plain][:, None] + np.arange(L, dtype=np.uint64)).reshape(-1)] = rows[plain].reshape(-1)
    flat[(off[idx][:, None] + np.arange(ov.shape[1], dtype=np.uint64)).reshape(-1)] = ov.reshape(-1)
    return flat, off.astype(np.uint32), idx


def pinned(a):
    """Copy a numpy array into pinned host memory (rl_alloc_host)."""
    if a is None:
        return None
    p = lib().rl_alloc_host(max(a.nbytes, 1))
    out = np.ctypeslib.as_array((C.c_uint8 * max(a.nbytes, 1)).from_address(p)).view(a.dtype)[:a.size]
    out[...] = a
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c1", choices=["c1", "c2"])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--requests", type=int, default=500_000)
    ap.add_argument("--tenants", type=int, default=10_000_000)
    ap.add_argument("--verdict", default="off", choices=["off", "full", "only"])
    ap.add_argument("--path", default="sync", choices=["sync", "packed-async", "wire-async"])
    ap.add_argument("--from-payloads", action="store_true")
    ap.add_argument("--pack-threads", type=int, default=1)
    ap.add_argument("--respond", action="store_true")
    ap.add_argument("--respond-headers", action="store_true")
    ap.add_argument("--override-share", type=float, default=0.0)
    ap.add_argument("--device-overrides", action="store_true")
    args = ap.parse_args()
    args.respond = args.respond or args.respond_headers
    keys = HEADER_KEYS if args.respond_headers else None
    if args.respond and (args.path != "wire-async" or args.from_payloads):
        ap.error("--respond goes with --path wire-async (buffers built in advance)")
    if args.from_payloads and args.path == "sync":
        ap.error("--from-payloads goes with --path packed-async or wire-async")
    if not 1 <= args.pack_threads <= 16:
        ap.error("--pack-threads: 1..16")
    share = args.override_share
    if (share or args.device_overrides) and not (args.path == "wire-async" and args.from_payloads):
        ap.error("--override-share / --device-overrides go with --path wire-async --from-payloads")
    if not 0.0 <= share <= 1.0:
        ap.error("--override-share: 0..1")
    nq, T = args.requests, args.tenants
    rng = np.random.default_rng(0xC1 if args.config == "c1" else 0xC2)
    zs = W.ZipfSampler(T, 1.1) if args.config == "c2" else None
    kw = dict(table_slots=1 << 26, max_batch=2 * nq, max_rules=16)
    if share or args.device_overrides:  # (rows for the override stats keys, on either flow)
        kw["max_rules"] = 2 + OVERRIDE_CAPACITY
    be_req = Backend(0.8, False, **kw)
    be_pk = Backend(0.8, False, **kw)
    tree = ConfigTree.from_yaml([("c1.yaml", W.C1_CONFIG_YAML)])
    be_req.load_config(tree)
    wire_rules = 2
    if args.device_overrides:
        be_req.enable_override_rules(2, OVERRIDE_CAPACITY)
        wire_rules = 2 + OVERRIDE_CAPACITY
    batches, payloads, var = [], [], []
    for b in range(4):
        t = zs.sample(rng, nq) if zs is not None else rng.integers(0, T, nq)
        h = rng.integers(1, 9, nq) if args.config == "c2" else None
        if args.path == "wire-async" or args.from_payloads:
            payloads.append(W.c1_payloads(t, h))  # (pageable: the bytes as the gRPC server received them)
            if share:
                var.append(override_payloads(payloads[-1], t, share, rng))
        raw = {k: pinned(v) for k, v in W.c1_requests(t, W.NOW0 + b, h).items()}
        pk, n, _, nr = W.c1_batch(t, W.NOW0 + b, h)
        batches.append((raw, {k: pinned(v) for k, v in pk.items()}, n))
    n = batches[0][2]
    # results (pinned)
    rr = {k: pinned(np.zeros(n, dt)) for k, dt in abi.REQUEST_RESULT_DTYPES.items()}
    rr["stats"] = pinned(np.zeros(2 * abi.RL_NUM_STATS, np.uint64))
    pr = {k: pinned(np.zeros(n, dt)) for k, dt in abi.RESULT_DTYPES.items() if k != "stats"}
    pr["stats"] = pinned(np.zeros(2 * abi.RL_NUM_STATS, np.uint64))

    vr = {k: pinned(np.zeros(nq, dt)) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
    vr["global_shadow"] = pinned(np.zeros(1, np.uint64))
    d2h = {"off": 0, "full": 18 * nq + 8, "only": 18 * nq + 8}[args.verdict]  # bytes per call, stats apart
    if args.verdict != "only":
        d2h += sum(v.nbytes for k, v in rr.items() if k != "stats")

    def req_call(raw):
        b = abi.RlRequestBatch()
        b.n_requests, b.n_descriptors, b.n_entries, b.n_rules = nq, n, 2 * n, 2
        for k in abi.REQUEST_ARRAYS:
            setattr(b, k, abi.ptr(raw[k]))
        r = abi.RlRequestResult()
        for k in rr:
            setattr(r, k, abi.ptr(rr[k]))
        if args.verdict == "off":
            rc = lib().rl_do_limit_requests(be_req.ctx, C.byref(b), C.byref(r))
        else:
            v = abi.RlRequestVerdict()
            for k in vr:
                setattr(v, k, abi.ptr(vr[k]))
            rp = C.byref(r) if args.verdict == "full" else None
            rc = lib().rl_do_limit_requests_verdict(be_req.ctx, C.byref(b), rp, 0, C.byref(v))
        assert rc == 0, lib().rl_last_error(be_req.ctx)

    def pk_call(pk):
        b = abi.make_batch_struct(pk, n, nq, 2)
        r = abi.make_result_struct(pr)
        rc = lib().rl_do_limit(be_pk.ctx, C.byref(b), C.byref(r))
        assert rc == 0, lib().rl_last_error(be_pk.ctx)

    # --path packed-async: the four batches in the one-buffer layout, PACKED_RING buffers and output sets
    ring, arena = [], PinnedArena()
    packed_bytes = None
    if hasattr(lib(), "rl_request_batch_pack"):
        packed_bytes = int(be_req.pack_requests(batches[0][0], 2).struct.buf_bytes)
    if args.path == "packed-async" and not args.from_payloads:
        for j in range(PACKED_RING):
            p = be_req.pack_requests(batches[j % 4][0], 2, arena)
            out = None
            if args.verdict != "only":
                out = {k: arena.array(n, dt) for k, dt in abi.REQUEST_RESULT_DTYPES.items()}
                out["stats"] = arena.array(2 * abi.RL_NUM_STATS, np.uint64)
            ver = None
            if args.verdict != "off":
                ver = {k: arena.array(nq, dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
                ver["global_shadow"] = arena.array(1, np.uint64)
            ring.append((p, out, ver, p.buf[p.struct.now:p.struct.now + 4 * nq].view(np.uint32)))

    def async_call(j, now):
        if args.path == "wire-async":
            return wire_call(j, now)
        p, out, ver, now32 = ring[j]
        now32[:] = now
        return be_req.do_limit_requests_packed_async(p, out, ver)

    # --path wire-async: PACKED_RING pinned wire buffers (offsets | clocks | payload bytes) and output sets
    wire_bytes = None
    if args.path == "wire-async":
        for j in range(PACKED_RING):
            if share:
                flat, off, _ = var[j % 4]
                raw = flat.tobytes()
                msgs = [raw[off[q]:off[q + 1]] for q in range(nq)]
            else:
                msgs = [r.tobytes() for r in payloads[j % 4]]
            wb = be_req.wire_batch(msgs, [W.NOW0] * nq, arena, wire_rules)
            wire_bytes = int(wb.struct.buf_bytes)
            out = None
            if args.verdict != "only":
                out = {k: arena.array(n, dt) for k, dt in abi.REQUEST_RESULT_DTYPES.items()}
                out["stats"] = arena.array(wire_rules * abi.RL_NUM_STATS, np.uint64)
            ver = None
            if args.verdict != "off":
                ver = {k: arena.array(nq, dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
                ver["global_shadow"] = arena.array(1, np.uint64)
            wire = {"req_status": arena.array(nq, np.uint8), "n_descriptors": arena.array(1, np.uint32)}
            resp = None
            if args.respond:
                if out is None or ver is None:
                    ap.error("--respond: the warm-up compares with the arrays (--verdict full)")
                wire["desc_first"] = arena.array(nq + 1, np.uint32)
                resp = {"bytes": arena.array(be_req.response_bound(nq, n, keys), np.uint8),
                        "resp_off": arena.array(nq + 1, np.uint32)}
            ws = wb.struct
            ring.append((wb, out, ver, wb.buf[ws.now:ws.now + 4 * nq].view(np.uint32), wire,
                         wb.buf[ws.msg_off:ws.msg_off + 4 * (nq + 1)].view(np.uint32),
                         wb.buf[ws.msgs:ws.msgs + ws.msgs_bytes], resp))
    L_msg = payloads[0].shape[1] if payloads else 0
    msg_off32 = (np.arange(nq + 1, dtype=np.uint64) * L_msg).astype(np.uint32)

    def wire_call(j, now, b=None, arrays=False):
        wb, out, ver, now32, wire, off32, body, resp = ring[j]
        if b is not None and share:  # --from-payloads: the host's work per batch
            body[:] = var[b][0]
            off32[:] = var[b][1]
        elif b is not None:
            body[:] = payloads[b].reshape(-1)
            off32[:] = msg_off32
        now32[:] = now
        if resp is not None:  # the timed loop takes the responses alone (and the stats); the warm-up the arrays too
            return be_req.do_limit_wire_respond_async(wb, wire, out if arrays else {"stats": out["stats"]},
                                                      ver if arrays else None, resp, keys, False, n)
        return be_req.do_limit_wire_async(wb, wire, out, ver, False, n)

    # --override-share without --device-overrides: the deferred messages of ring[j]'s completed batch (batch b's
    # payloads) through the host packer and the synchronous request path
    defer_flow = bool(share) and not args.device_overrides
    rs = {}
    if defer_flow:
        m_max = max(len(v[2]) for v in var)
        ov_len = int(var[0][1][var[0][2][0] + 1] - var[0][1][var[0][2][0]])
        rs = dict(packer=lib().rl_packer_create(2), rb=abi.RlRequestBatch(), nows=np.zeros(m_max, np.int64),
                  off=np.arange(m_max + 1, dtype=np.uint64) * ov_len, span=np.arange(ov_len, dtype=np.uint64),
                  out={k: pinned(np.zeros(2 * m_max, dt)) for k, dt in abi.REQUEST_RESULT_DTYPES.items()})
        rs["out"]["stats"] = pinned(np.zeros((2 + OVERRIDE_CAPACITY) * abi.RL_NUM_STATS, np.uint64))

    def resubmit(j, b, now):
        L = lib()
        status = ring[j][4]["req_status"]
        idx = np.nonzero(status[:nq] == abi.RL_WIRE_DEFERRED)[0]
        if not len(idx):
            return 0
        flat, off, _ = var[b]
        body = flat[(off[idx].astype(np.uint64)[:, None] + rs["span"]).reshape(-1)]
        rs["nows"][:len(idx)] = now
        rc = L.rl_packer_pack(rs["packer"], abi.ptr(body), abi.ptr(rs["off"]), len(idx), abi.ptr(rs["nows"]),
                              C.byref(rs["rb"]))
        assert rc == 0
        assert rs["rb"].n_rules <= 2 + OVERRIDE_CAPACITY
        r = abi.RlRequestResult()
        for k in rs["out"]:
            setattr(r, k, abi.ptr(rs["out"][k]))
        rc = L.rl_do_limit_requests(be_req.ctx, C.byref(rs["rb"]), C.byref(r))
        assert rc == 0, L.rl_last_error(be_req.ctx)
        return len(idx)

    def host_serialize(j, threads, reps=5):
        """rl_response_serialize over ring[j]'s arrays, one contiguous slice of the requests per thread
        -> [seconds] per repetition."""
        from concurrent.futures import ThreadPoolExecutor
        L = lib()
        _, out, ver, _, wire, _, _, resp = ring[j]
        first = wire["desc_first"][:nq + 1]
        f, keep = abi.make_response_format(keys)
        jobs = []
        for k in range(threads):
            q0, q1 = nq * k // threads, nq * (k + 1) // threads
            d0 = int(first[q0])
            r, v = abi.RlRequestResult(), abi.RlRequestVerdict()
            for key in abi.REQUEST_RESULT_DTYPES:
                setattr(r, key, abi.ptr(out[key][d0:]))
            for key in abi.REQUEST_VERDICT_DTYPES:
                setattr(v, key, abi.ptr(ver[key][q0:]))
            fs = (first[q0:q1 + 1] - first[q0]).astype(np.uint32)
            cap = be_req.response_bound(q1 - q0, int(fs[-1]), keys)
            jobs.append((q1 - q0, fs, r, v, np.zeros(cap, np.uint8), cap, np.zeros(q1 - q0 + 1, np.uint32),
                         C.c_uint64(0)))

        def one(job):
            m, fs, r, v, buf, cap, off, need = job
            rc = L.rl_response_serialize(m, abi.ptr(fs), None, C.byref(r), C.byref(v), C.byref(f), abi.ptr(buf), cap,
                                         abi.ptr(off), C.byref(need))
            assert rc == 0, rc
            return int(need.value)

        times = []
        with ThreadPoolExecutor(threads) as ex:
            for _ in range(reps):
                t0 = time.perf_counter()
                total = sum(ex.map(one, jobs))
                times.append(time.perf_counter() - t0)
        assert total == int(resp["resp_off"][nq])
        return times

    # --from-payloads on packed-async: each batch's messages split over the pack threads, every slice
    # parsed (rl_packer_pack) and laid out (rl_request_batch_pack) by its thread, then submitted
    NT = args.pack_threads
    pack_ring, pool = [], None
    if args.from_payloads and args.path == "packed-async":
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(NT)
        cut = [nq * k // NT for k in range(NT + 1)]
        L = lib()
        for j in range(PACKED_RING):
            slots = []
            for k in range(NT):
                m = cut[k + 1] - cut[k]
                probe = be_req.pack_requests(W.c1_requests(np.zeros(m, np.int64), W.NOW0), 2)  # (its size)
                size = int(probe.struct.buf_bytes)
                out = None
                if args.verdict != "only":
                    out = {key: arena.array(2 * m, dt) for key, dt in abi.REQUEST_RESULT_DTYPES.items()}
                    out["stats"] = arena.array(2 * abi.RL_NUM_STATS, np.uint64)
                ver = None
                if args.verdict != "off":
                    ver = {key: arena.array(m, dt) for key, dt in abi.REQUEST_VERDICT_DTYPES.items()}
                    ver["global_shadow"] = arena.array(1, np.uint64)
                slots.append(dict(buf=arena.array(size, np.uint8), size=size, out=out, ver=ver,
                                  packer=L.rl_packer_create(2), rb=abi.RlRequestBatch(),
                                  p=abi.RlRequestBatchPacked(), nows=np.zeros(m, np.int64),
                                  off=(np.arange(m + 1, dtype=np.uint64) * L_msg), m=m))
            pack_ring.append(slots)

        def pack_slice(sl, body, now):
            sl["nows"][:] = now
            rc = L.rl_packer_pack(sl["packer"], abi.ptr(body), abi.ptr(sl["off"]), sl["m"], abi.ptr(sl["nows"]),
                                  C.byref(sl["rb"]))
            assert rc == 0
            sl["rb"].n_rules = 2
            rc = L.rl_request_batch_pack(C.byref(sl["rb"]), abi.ptr(sl["buf"]), sl["size"], C.byref(sl["p"]))
            assert rc == 0, rc
            return sl

    def packed_from_payloads(j, b, now):
        from ratelimit_amd.limiter import PackedRequests
        flat = payloads[b].reshape(-1)
        futs = [pool.submit(pack_slice, sl, flat[cut[k] * L_msg:cut[k + 1] * L_msg], now)
                for k, sl in enumerate(pack_ring[j])]
        keep = []
        for f in futs:  # (submitted in slice order, as each is ready)
            sl = f.result()
            keep.append(be_req.do_limit_requests_packed_async(
                PackedRequests(sl["p"], sl["buf"], sl["m"], 2 * sl["m"], 2), sl["out"], sl["ver"]))
        return keep

    # warm-up + equality of the two paths on the same stream (clock +1 s per step)
    for s in range(8 if args.path == "sync" else 0):
        raw, pk, _ = batches[s % 4]
        now = W.NOW0 + s
        raw["now"][:] = now
        pk["now"][:] = now
        req_call(raw)
        pk_call(pk)
        if args.verdict != "only":
            for k in ("code", "limit_remaining", "reset_s"):
                assert np.array_equal(rr[k], pr[k]), k
            assert np.array_equal(rr["stats"], pr["stats"])
            assert (rr["match"] == abi.RL_MATCH_LIMIT).all()
        if args.verdict != "off":  # the overall code against the packed path's per-descriptor codes
            want = np.ones(nq, np.uint8)
            np.maximum.at(want, raw["req_idx"], pr["code"])
            assert np.array_equal(vr["overall_code"], want), "overall_code"
    sub_batches = NT if pack_ring else 1  # packed batches submitted per step
    for s in range(8 if args.path != "sync" else 0):
        pk = batches[s % 4][1]
        pk["now"][:] = W.NOW0 + s
        if pack_ring:
            packed_from_payloads(s % PACKED_RING, s % 4, W.NOW0 + s)
        elif args.from_payloads:
            wire_call(s % PACKED_RING, W.NOW0 + s, s % 4)
        elif args.respond:
            wire_call(s % PACKED_RING, W.NOW0 + s, arrays=True)
        else:
            async_call(s % PACKED_RING, W.NOW0 + s)
        be_req.synchronize()
        pk_call(pk)
        if pack_ring:  # the slices' outputs side by side are the batch's
            sl = pack_ring[s % PACKED_RING]
            out = ver = None
            if sl[0]["out"] is not None:
                out = {k: np.concatenate([x["out"][k][:2 * x["m"]] for x in sl]) for k in abi.REQUEST_RESULT_DTYPES}
                out["stats"] = np.sum([x["out"]["stats"] for x in sl], axis=0)
            if sl[0]["ver"] is not None:
                ver = {"overall_code": np.concatenate([x["ver"]["overall_code"][:x["m"]] for x in sl])}
        else:
            out, ver = ring[s % PACKED_RING][1:3]
        if args.path == "wire-async" and defer_flow:  # exactly the override requests are deferred
            wire = ring[s % PACKED_RING][4]
            assert np.array_equal(np.nonzero(wire["req_status"][:nq])[0], var[s % 4][2])
            assert resubmit(s % PACKED_RING, s % 4, W.NOW0 + s) == len(var[s % 4][2])
            continue
        if args.path == "wire-async":
            wire = ring[s % PACKED_RING][4]
            assert not wire["req_status"].any() and int(wire["n_descriptors"][0]) == n
        if share:  # (the overrides change the limits: no parity with the packed DoLimit path)
            assert (out["match"] == abi.RL_MATCH_LIMIT).all() if out is not None else True
            continue
        if args.respond:  # the device's bytes are the host twin's over the returned arrays
            resp = ring[s % PACKED_RING][7]
            raw, off = be_req.response_serialize(wire["desc_first"][:nq + 1], None, out, ver, keys)
            assert np.array_equal(off, resp["resp_off"][:nq + 1]), "resp_off"
            assert np.array_equal(raw, resp["bytes"][:len(raw)]), "response bytes"
            d2h = len(raw) + 4 * (nq + 1)  # the responses and their offsets
        if out is not None:
            for k in ("code", "limit_remaining", "reset_s"):
                assert np.array_equal(out[k], pr[k]), k
            assert np.array_equal(out["stats"], pr["stats"])
            assert (out["match"] == abi.RL_MATCH_LIMIT).all()
        if ver is not None:
            want = np.ones(nq, np.uint8)
            np.maximum.at(want, batches[s % 4][0]["req_idx"], pr["code"])
            assert np.array_equal(ver["overall_code"], want), "overall_code"
    host_ms = resp_bytes = None
    if args.respond:  # the host step the device replaces, on the last warm-up batch's arrays
        resp_bytes = int(ring[7 % PACKED_RING][7]["resp_off"][nq])
        host_ms = {str(t): [round(1e3 * x, 3) for x in host_serialize(7 % PACKED_RING, t)] for t in (1, 4, 16)}
    res = {}
    if args.path != "sync":
        base = be_req.batch_progress()[0]
        keep = []
        resubmitted = 0
        t0 = time.perf_counter()
        for s in range(args.steps):
            # the buffer's previous batch is complete
            while be_req.batch_progress()[1] - base + PACKED_RING * sub_batches <= s * sub_batches:
                pass
            if defer_flow and s >= PACKED_RING:  # the buffer's completed batch: its deferred messages, on the host
                resubmitted += resubmit(s % PACKED_RING, s % 4, W.NOW0 + 8 + s - PACKED_RING)
            if pack_ring:
                keep.append(packed_from_payloads(s % PACKED_RING, s % 4, W.NOW0 + 8 + s))
            elif args.from_payloads:
                keep.append(wire_call(s % PACKED_RING, W.NOW0 + 8 + s, s % 4))
            else:
                keep.append(async_call(s % PACKED_RING, W.NOW0 + 8 + s))
        be_req.synchronize()
        for s in range(max(args.steps - PACKED_RING, 0), args.steps if defer_flow else 0):  # the last batches' deferred
            resubmitted += resubmit(s % PACKED_RING, s % 4, W.NOW0 + 8 + s)
        res["requests"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        for s in range(args.steps):
            bt = batches[s % 4][1]
            bt["now"][:] = W.NOW0 + 8 + s
            pk_call(bt)
        res["packed"] = time.perf_counter() - t0
    for name, fn, idx in (("requests", req_call, 0), ("packed", pk_call, 1)) if args.path == "sync" else ():
        t0 = time.perf_counter()
        for s in range(args.steps):
            bt = batches[s % 4][idx]
            bt["now"][:] = W.NOW0 + 8 + s
            fn(bt)
        res[name] = time.perf_counter() - t0
    path = "rl_do_limit_requests" if args.verdict == "off" else "rl_do_limit_requests_verdict"
    if args.path == "packed-async":
        path = "rl_do_limit_requests_packed_async"
    if args.path == "wire-async":
        path = "rl_do_limit_wire_respond_async" if args.respond else "rl_do_limit_wire_async"
    out = {"path": path + " (host buffers, PCIe-inclusive)", "config": args.config.upper(),
           "verdict": args.verdict, "d2h_bytes_per_descriptor": d2h / n,
           "descriptors_per_batch": n, "steps": args.steps,
           "requests_decisions_per_s": n * args.steps / res["requests"],
           "requests_ms_per_batch": 1e3 * res["requests"] / args.steps,
           "packed_decisions_per_s": n * args.steps / res["packed"],
           "packed_ms_per_batch": 1e3 * res["packed"] / args.steps,
           "raw_bytes_per_descriptor": sum(v.nbytes for v in batches[0][0].values() if v is not None) / n,
           "packed_bytes_per_descriptor": sum(v.nbytes for v in batches[0][1].values()) / n,
           "parity": "request path == packed DoLimit path on 8 warm-up batches"}
    if packed_bytes is not None:  # the one-buffer layout of the same batch (rl_request_batch_pack)
        out["packed_request_bytes_per_descriptor"] = packed_bytes / n
    if args.path != "sync":
        out["path"] = path + " (one pinned buffer per batch, pipelined, PCIe-inclusive)"
        out["h2d_bytes_per_descriptor"] = (wire_bytes if args.path == "wire-async" else packed_bytes) / n
        out["from_payloads"] = bool(args.from_payloads)
        if pack_ring:
            out["pack_threads"] = NT
    if share or args.device_overrides:
        out["override_share"] = share
        out["device_overrides"] = bool(args.device_overrides)
        out["override_requests_per_batch"] = [int(len(v[2])) for v in var]
        out["parity"] = "skipped (overrides change the limits); warm-up checks the statuses"
        if defer_flow:
            out["resubmitted_requests"] = resubmitted
        else:
            out["override_rules"] = be_req.override_rules_info() if args.device_overrides else None
    if args.respond:
        out["respond"] = True
        out["response_headers"] = bool(args.respond_headers)
        out["response_bytes_per_descriptor"] = resp_bytes / n
        out["host_serialize_ms"] = host_ms  # rl_response_serialize per batch on 1, 4, 16 threads, each repetition
    print(json.dumps(out))


if __name__ == "__main__":
    main()
