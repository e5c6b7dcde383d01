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

    python scripts/bench_requests.py [--config c1|c2] [--steps K] [--verdict off|full|only]
                                     [--path sync|packed-async]
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
    ap.add_argument("--path", default="sync", choices=["sync", "packed-async"])
    args = ap.parse_args()
    nq, T = args.requests, args.tenants
    rng = np.random.default_rng(0xC1 if args.config == "c1" else 0xC2)
    zs = W.ZipfSampler(T, 1.1) if args.config == "c2" else None
    kw = dict(table_slots=1 << 26, max_batch=2 * nq, max_rules=16)
    be_req = Backend(0.8, False, **kw)
    be_pk = Backend(0.8, False, **kw)
    tree = ConfigTree.from_yaml([("c1.yaml", W.C1_CONFIG_YAML)])
    be_req.load_config(tree)
    batches = []
    for b in range(4):
        t = zs.sample(rng, nq) if zs is not None else rng.integers(0, T, nq)
        h = rng.integers(1, 9, nq) if args.config == "c2" else None
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
    if args.path == "packed-async":
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
        p, out, ver, now32 = ring[j]
        now32[:] = now
        return be_req.do_limit_requests_packed_async(p, out, ver)

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
    for s in range(8 if args.path == "packed-async" else 0):
        pk = batches[s % 4][1]
        pk["now"][:] = W.NOW0 + s
        async_call(s % PACKED_RING, W.NOW0 + s)
        be_req.synchronize()
        pk_call(pk)
        _, out, ver, _ = ring[s % PACKED_RING]
        if out is not None:
            for k in ("code", "limit_remaining", "reset_s"):
                assert np.array_equal(out[k], pr[k]), k
            assert np.array_equal(out["stats"], pr["stats"])
            assert (out["match"] == abi.RL_MATCH_LIMIT).all()
        if ver is not None:
            want = np.ones(nq, np.uint8)
            np.maximum.at(want, batches[s % 4][0]["req_idx"], pr["code"])
            assert np.array_equal(ver["overall_code"], want), "overall_code"
    res = {}
    if args.path == "packed-async":
        base = be_req.batch_progress()[0]
        keep = []
        t0 = time.perf_counter()
        for s in range(args.steps):
            while be_req.batch_progress()[1] - base + PACKED_RING <= s:  # the buffer's previous batch is complete
                pass
            keep.append(async_call(s % PACKED_RING, W.NOW0 + 8 + s))
        be_req.synchronize()
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
    if args.path == "packed-async":
        out["path"] = path + " (one pinned buffer per batch, pipelined, PCIe-inclusive)"
        out["h2d_bytes_per_descriptor"] = packed_bytes / n
    print(json.dumps(out))


if __name__ == "__main__":
    main()
