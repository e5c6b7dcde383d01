"""Host-side mirror of the reference's RateLimitCache interface over the C ABI.

``GpuRateLimitCache`` is what a user of the reference's
``limiter.RateLimitCache`` (src/limiter/cache.go:11-29) switches to:

    cache = GpuRateLimitCache(time_source, near_limit_ratio=0.8, local_cache=True,
                              cache_key_prefix="", per_second=False)
    statuses = cache.do_limit(ctx, request, limits)   # DoLimit
    cache.flush()                                     # Flush

Same argument meaning and error behaviour as
``redis.NewFixedRateLimitCacheImpl`` / ``fixedRateLimitCacheImpl.DoLimit``
(src/redis/fixed_cache_impl.go:33-125): nil limits answer {OK, nil, 0}; the
per-rule stats counters (limit.stats) are incremented; backend failures raise
``RedisError`` (the reference panics with redis.RedisError).  ``do_limit_batch``
is the batcher's entry point: many in-flight calls, one GPU launch sequence.
"""
import ctypes as C
import time
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import abi
from ._lib import RedisError, check, lib, load
from .packing import PackedBatch, RuleInterner, pack_calls
from .types import OK, DescriptorStatus, Limit  # noqa: F401  (re-exported data model)

# rl_profile stages (include/ratelimit_hip.h RL_NUM_STAGES)
STAGES = ("prepare", "sort", "segment", "table", "finish")
PROFILE_FIELDS = STAGES + ("table_kernel",)  # + k_table's own run time (device clock)

__all__ = ["GpuRateLimitCache", "GpuRateLimitService", "HotKey", "KeyState", "RedisError", "RequestVerdict", "TimeSource",
           "migrate"]


class KeyState(NamedTuple):
    """One Redis key as GpuRateLimitCache.peek reads it: GET's value (0 when the
    key does not exist), its TTL in seconds (None: no such key) and whether the
    local over-limit cache holds it."""
    count: int
    ttl_s: Optional[int]
    over_limit_cached: bool


class HotKey(NamedTuple):
    """One record of GpuRateLimitCache.hot_keys: the key's stem and unit, its
    window's start, counter and expiry, and the expiry of its local over-limit
    cache entry (0: none)."""
    stem: bytes
    unit: int
    ws: int
    count: int
    expire: int
    lc: int


class TimeSource:
    """utils.TimeSource (src/utils/utilities.go:9-12)."""

    def unix_now(self) -> int:
        return int(time.time())


class FixedTimeSource(TimeSource):
    def __init__(self, now: int):
        self.now = now

    def unix_now(self) -> int:
        return self.now


def _config(near_limit_ratio, local_cache, per_second, jitter, table_slots, max_batch, max_rules, device,
            arena_bytes, max_stem_bytes, hash_seed=0, debug_hash_bits=0, n_shards=1, shard_devices=None,
            history_entries=0):
    cfg = abi.RlConfig()
    cfg.history_entries = history_entries
    cfg.table_slots = table_slots
    cfg.arena_bytes = arena_bytes
    cfg.max_batch = max_batch
    cfg.max_requests = max_batch
    cfg.max_rules = max_rules
    cfg.max_stem_bytes = max_stem_bytes
    cfg.near_limit_ratio = near_limit_ratio
    cfg.local_cache_enabled = 1 if local_cache else 0
    cfg.per_second_split = 1 if per_second else 0
    cfg.device = device
    cfg.expiration_jitter_max_seconds = jitter
    cfg.hash_seed = hash_seed
    cfg.debug_hash_bits = debug_hash_bits
    cfg.n_shards = n_shards
    devs = list(shard_devices) if shard_devices is not None else [device] * n_shards
    if len(devs) != n_shards or n_shards > 16:
        raise ValueError("shard_devices must name n_shards (<= 16) devices")
    for j, d in enumerate(devs):
        cfg.shard_device[j] = d
    return cfg


class PinnedArena:
    """Page-locked host arrays from the library (rl_alloc_host): numpy views
    whose PCIe copies run asynchronously (rl_do_limit_host_async)."""

    def __init__(self):
        self.ptrs = []

    def array(self, n: int, dtype) -> np.ndarray:
        dt = np.dtype(dtype)
        nbytes = max(int(n), 1) * dt.itemsize
        p = lib().rl_alloc_host(nbytes)
        if not p:
            raise MemoryError("rl_alloc_host(%d) failed" % nbytes)
        self.ptrs.append(p)
        buf = (C.c_uint8 * nbytes).from_address(p)
        return np.frombuffer(buf, dtype=dt, count=max(int(n), 1))

    def like(self, a: np.ndarray) -> np.ndarray:
        out = self.array(a.size, a.dtype)
        out[:a.size] = a
        return out

    def close(self):
        for p in self.ptrs:
            lib().rl_free_host(p)
        self.ptrs = []


class PackedRequests(NamedTuple):
    """A request batch in the one-buffer layout (Backend.pack_requests)."""
    struct: object                  # abi.RlRequestBatchPacked (its buf points into ``buf``)
    buf: np.ndarray                 # the buffer: pinned when packed into a PinnedArena
    n_requests: int
    n_descriptors: int
    n_rules: int


class WireRequests(NamedTuple):
    """Serialized RateLimitRequest payloads in the one-buffer layout of rl_wire_batch (Backend.wire_batch)."""
    struct: object                  # abi.RlWireBatch (its buf points into ``buf``)
    buf: np.ndarray                 # the buffer: pinned when built in a PinnedArena
    n_requests: int
    msgs_bytes: int


class Backend:
    """Owns one rl_ctx (one GPU's table)."""

    def __init__(self, near_limit_ratio=0.8, local_cache=False, per_second=False, jitter=0,
                 table_slots=1 << 20, max_batch=1 << 16, max_rules=1 << 12, device=0, arena_bytes=0,
                 max_stem_bytes=0, hash_seed=0, debug_hash_bits=0, n_shards=1, shard_devices=None, history_entries=0,
                 library=None):
        """n_shards > 1: one ctx hash-shards its table over shard_devices (default:
        all on `device`) and routes every batch between them (rl_config.n_shards).
        history_entries: 32-B history log entries (0 = table_slots; rl_config.history_entries).
        jitter: EXPIRATION_JITTER_MAX_SECONDS (the history horizon: older windows kept div + jitter s).
        library: a path to another build of the library (tests: the RL_LOG_TEAR build); default the product's."""
        L = self.L = lib() if library is None else load(library)
        err = C.create_string_buffer(512)
        self.cfg = _config(near_limit_ratio, local_cache, per_second, jitter, table_slots, max_batch, max_rules,
                           device, arena_bytes, max_stem_bytes, hash_seed, debug_hash_bits, n_shards, shard_devices,
                           history_entries)
        self.ctx = L.rl_create(C.byref(self.cfg), err, 512)
        if not self.ctx:
            raise RedisError(err.value.decode())

    def _check(self, rc):
        check(self.ctx, rc, self.L)

    def close(self):
        if getattr(self, "ctx", None):
            self.L.rl_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- raw packed-batch entry points
    def do_limit_packed(self, pb: PackedBatch, isolate: bool = False):
        """rl_do_limit. isolate: per-descriptor statuses (result "status"): a
        descriptor that cannot be answered fails alone instead of the batch."""
        out = pb.alloc_result(isolate)
        b = pb.batch_struct()
        r = abi.make_result_struct(out)
        self._check(self.L.rl_do_limit(self.ctx, C.byref(b), C.byref(r)))
        n, nr = pb.n, pb.n_rules
        res = {"code": out["code"][:n], "limit_remaining": out["limit_remaining"][:n],
               "reset_s": out["reset_s"][:n], "stats": out["stats"][:nr * abi.RL_NUM_STATS]}
        if isolate:
            res["status"] = out["status"][:n]
        return res

    def do_limit_arrays(self, arrays, n, n_requests, n_rules, isolate: bool = False):
        return self.do_limit_packed(PackedBatch(arrays, n, n_requests, n_rules), isolate)

    def do_limit_device(self, dev_in: dict, dev_out: dict, n, n_requests, n_rules, stream=None):
        """All arrays are torch CUDA tensors (device memory); asynchronous and
        pipelined; dev_out is read after synchronize(). `stream` (a hipStream_t
        handle; default: torch's current stream) orders the batch after the
        work producing its inputs. torch's default stream has the NULL handle,
        which the library cannot order against cheaply: under it, the inputs
        must be complete at the call."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        b = abi.make_batch_struct(dev_in, n, n_requests, n_rules)
        r = abi.make_result_struct(dev_out)
        self._check(self.L.rl_do_limit_async(self.ctx, C.byref(b), C.byref(r),
                                                C.c_void_p(stream) if stream else None))

    def do_limit_structs(self, b, r, stream=None):
        """rl_do_limit_async with prebuilt rl_batch / rl_result structs (device
        arrays; the structs are read during the call only): what a C or Go
        caller does per batch. stream: a hipStream_t handle, or None (the
        inputs are complete at the call)."""
        self._check(self.L.rl_do_limit_async(self.ctx, C.byref(b), C.byref(r), C.c_void_p(stream) if stream else None))

    def do_limit_host_async(self, pb: PackedBatch, out: dict):
        """rl_do_limit_host_async: host arrays in (pb) and out (dict of numpy
        arrays: code, limit_remaining, reset_s, stats[, status]), nothing waited
        for; out is final after synchronize(). Both must stay alive and
        untouched until then; pinned arrays (PinnedArena) make the copies
        asynchronous."""
        b = pb.batch_struct()
        r = abi.make_result_struct(out)
        self._check(self.L.rl_do_limit_host_async(self.ctx, C.byref(b), C.byref(r)))
        return b, r  # (the structs the call read; kept by the caller with the arrays)

    def do_limit_compact_async(self, cb, out: dict):
        """rl_do_limit_compact_async: a CompactBatch (packing.compact_batch; its
        buffer pinned for an asynchronous copy) in, out as do_limit_host_async;
        final after synchronize()."""
        r = abi.make_result_struct(out)
        s = cb.struct()
        self._check(self.L.rl_do_limit_compact_async(self.ctx, C.byref(s), C.byref(r)))
        return s, r

    def batch_progress(self):
        """rl_batch_progress: (batches submitted, batches complete), never waits."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.rl_batch_progress(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def do_limit_prefixed_async(self, pb, out: dict):
        """rl_do_limit_prefixed_async: a PrefixedBatch (packing.prefixed_batch;
        its buffer pinned for an asynchronous copy) in, out as
        do_limit_host_async; final after synchronize()."""
        r = abi.make_result_struct(out)
        s = pb.struct()
        self._check(self.L.rl_do_limit_prefixed_async(self.ctx, C.byref(s), C.byref(r)))
        return s, r

    # ---- config match + DoLimit on raw requests (rl_match.hip)
    def load_config(self, tree) -> None:
        """rl_config_load: ``tree`` is a ratelimit_amd.config.ConfigTree."""
        nodes, kb, pre = tree.arrays()
        t = abi.RlConfigTree()
        t.n_nodes = len(nodes)
        t.cache_key_prefix_len = len(tree.prefix.encode())
        t.nodes = C.c_void_p(nodes.ctypes.data)
        t.key_bytes = abi.ptr(kb)
        t.key_bytes_len = sum(len(k) for k in tree.keys)
        t.cache_key_prefix = abi.ptr(pre)
        self._check(self.L.rl_config_load(self.ctx, C.byref(t)))

    def do_limit_requests(self, arrays: dict, n_rules: int) -> dict:
        """rl_do_limit_requests on pack_requests() arrays -> per-descriptor results + stats."""
        n = len(arrays["req_idx"])
        b = abi.RlRequestBatch()
        b.n_requests, b.n_descriptors, b.n_entries, b.n_rules = len(arrays["hits"]), n, len(arrays["key_len"]), n_rules
        for k in abi.REQUEST_ARRAYS:
            setattr(b, k, abi.ptr(arrays[k]))
        return self.do_limit_request_batch(b)

    def do_limit_request_batch(self, b) -> dict:
        """rl_do_limit_requests on a filled RlRequestBatch (e.g. from RequestPacker.pack)."""
        n, n_rules = b.n_descriptors, b.n_rules
        out = {k: np.zeros(max(n, 1), dt) for k, dt in abi.REQUEST_RESULT_DTYPES.items()}
        out["stats"] = np.zeros(max(n_rules, 1) * abi.RL_NUM_STATS, np.uint64)
        r = abi.RlRequestResult()
        for k in out:
            setattr(r, k, abi.ptr(out[k]))
        self._check(self.L.rl_do_limit_requests(self.ctx, C.byref(b), C.byref(r)))
        res = {k: v[:n] for k, v in out.items() if k != "stats"}
        res["stats"] = out["stats"][:n_rules * abi.RL_NUM_STATS]
        return res

    def do_limit_requests_verdict(self, arrays: dict, n_rules: int, global_shadow: bool = False,
                                  per_descriptor: bool = True, stats: bool = True) -> dict:
        """rl_do_limit_requests_verdict on pack_requests() arrays -> the per-request
        verdict arrays (abi.REQUEST_VERDICT_DTYPES) and ``global_shadow`` (this
        call's count), with do_limit_requests' per-descriptor arrays when
        ``per_descriptor`` and the per-rule ``stats`` deltas when ``stats``; with
        neither, ``out`` is NULL and only per-request bytes come back."""
        n, nq = len(arrays["req_idx"]), len(arrays["hits"])
        b = abi.RlRequestBatch()
        b.n_requests, b.n_descriptors, b.n_entries, b.n_rules = nq, n, len(arrays["key_len"]), n_rules
        for k in abi.REQUEST_ARRAYS:
            setattr(b, k, abi.ptr(arrays[k]))
        out = {}
        if per_descriptor:
            out = {k: np.zeros(max(n, 1), dt) for k, dt in abi.REQUEST_RESULT_DTYPES.items()}
        if stats:
            out["stats"] = np.zeros(max(n_rules, 1) * abi.RL_NUM_STATS, np.uint64)
        r = abi.RlRequestResult()
        for k in out:
            setattr(r, k, abi.ptr(out[k]))
        ver = {k: np.zeros(max(nq, 1), dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
        gs = np.zeros(1, np.uint64)
        v = abi.RlRequestVerdict()
        for k in ver:
            setattr(v, k, abi.ptr(ver[k]))
        v.global_shadow = abi.ptr(gs)
        opts = abi.RL_VERDICT_OPT_GLOBAL_SHADOW if global_shadow else 0
        self._check(self.L.rl_do_limit_requests_verdict(self.ctx, C.byref(b), C.byref(r) if out else None, opts,
                                                         C.byref(v)))
        res = {k: a[:n] for k, a in out.items() if k != "stats"}
        if stats:
            res["stats"] = out["stats"][:n_rules * abi.RL_NUM_STATS]
        res.update({k: a[:nq] for k, a in ver.items()})
        res["global_shadow"] = int(gs[0])
        return res

    def pack_requests(self, arrays: dict, n_rules: int, arena: Optional[PinnedArena] = None) -> PackedRequests:
        """rl_request_batch_pack: pack_requests() arrays -> the one-buffer layout
        of rl_do_limit_requests_packed_async, in a buffer from ``arena`` (pinned:
        the copy is asynchronous) or, without one, in pageable memory."""
        n, nq = len(arrays["req_idx"]), len(arrays["hits"])
        b = abi.RlRequestBatch()
        b.n_requests, b.n_descriptors, b.n_entries, b.n_rules = nq, n, len(arrays["key_len"]), n_rules
        for k in abi.REQUEST_ARRAYS:
            setattr(b, k, abi.ptr(arrays[k]))
        p = abi.RlRequestBatchPacked()
        rc = self.L.rl_request_batch_pack(C.byref(b), None, 0, C.byref(p))
        if rc != abi.RL_E_CAPACITY:
            raise RedisError("rl_request_batch_pack: malformed request batch [%s]" % abi.STATUS_NAMES.get(rc, rc), rc)
        size = int(p.buf_bytes)
        buf = arena.array(size, np.uint8) if arena is not None else np.zeros(max(size, 1), np.uint8)
        rc = self.L.rl_request_batch_pack(C.byref(b), abi.ptr(buf), size, C.byref(p))
        if rc:
            raise RedisError("rl_request_batch_pack failed [%s]" % abi.STATUS_NAMES.get(rc, rc), rc)
        return PackedRequests(p, buf, nq, n, n_rules)

    def do_limit_requests_packed_async(self, packed: PackedRequests, out: Optional[dict], verdict: Optional[dict],
                                       global_shadow: bool = False):
        """rl_do_limit_requests_packed_async: nothing waited for. ``out``: numpy
        arrays by rl_request_result field (any subset; None: no per-descriptor
        bytes come back); ``verdict``: numpy arrays by rl_request_verdict field
        (``global_shadow``: one uint64). Both are final after synchronize(), or
        once batch_progress() counts the batch complete; they and ``packed``
        must stay alive and untouched until then."""
        r = v = None
        if out is not None:
            r = abi.RlRequestResult()
            for k in out:
                setattr(r, k, abi.ptr(out[k]))
        if verdict is not None:
            v = abi.RlRequestVerdict()
            for k in verdict:
                setattr(v, k, abi.ptr(verdict[k]))
        opts = abi.RL_VERDICT_OPT_GLOBAL_SHADOW if global_shadow else 0
        self._check(self.L.rl_do_limit_requests_packed_async(self.ctx, C.byref(packed.struct),
                                                              C.byref(r) if r is not None else None, opts,
                                                              C.byref(v) if v is not None else None))
        return r, v

    @staticmethod
    def wire_batch(msgs, nows, arena: Optional[PinnedArena] = None, n_rules: int = 1) -> WireRequests:
        """Serialized RateLimitRequest payloads (``msgs``: bytes objects) and one
        UnixNow() per request -> the one-buffer layout of rl_do_limit_wire_async:
        [msg_off u32 x (n + 1) | now u32 x n | payload bytes], each section 4-byte
        aligned, in a buffer from ``arena`` (pinned: the copy is asynchronous) or,
        without one, in pageable memory. The payloads are only copied: numpy
        alone, no parsing."""
        nq = len(msgs)
        lens = np.fromiter((len(m) for m in msgs), np.uint64, nq)
        total = int(lens.sum())
        if total >= 1 << 32:
            raise RedisError("wire batch: payload bytes do not fit 32 bits", abi.RL_E_CAPACITY)
        o_off, o_now = 0, 4 * (nq + 1)
        o_msgs = o_now + 4 * nq
        size = (o_msgs + total + 3) & ~3
        buf = arena.array(size, np.uint8) if arena is not None else np.zeros(max(size, 1), np.uint8)
        off = buf[o_off:o_now].view(np.uint32)
        off[0] = 0
        np.cumsum(lens, out=off[1:], dtype=np.uint32)
        buf[o_now:o_msgs].view(np.uint32)[:] = np.asarray(nows, np.int64).astype(np.uint32)
        buf[o_msgs:o_msgs + total] = np.frombuffer(b"".join(msgs), np.uint8)
        buf[o_msgs + total:size] = 0
        w = abi.RlWireBatch()
        w.n_requests, w.n_rules = nq, n_rules
        w.buf, w.buf_bytes = abi.ptr(buf), size
        w.msg_off, w.now, w.msgs, w.msgs_bytes = o_off, o_now, o_msgs, total
        return WireRequests(w, buf, nq, total)

    def do_limit_wire_async(self, wb: WireRequests, wire: dict, out: Optional[dict], verdict: Optional[dict],
                            global_shadow: bool = False, desc_cap: Optional[int] = None):
        """rl_do_limit_wire_async: nothing waited for. ``wire``: numpy arrays
        ``req_status`` (uint8 per request; required), ``desc_first`` (uint32 x
        (n + 1)) and ``n_descriptors`` (one uint32), the latter two optional;
        ``out`` and ``verdict`` as for do_limit_requests_packed_async, ``out``'s
        per-descriptor arrays holding ``desc_cap`` descriptors (default: the
        length of the shortest). All are final after synchronize(), or once
        batch_progress() counts the batch complete; they and ``wb`` must stay
        alive and untouched until then."""
        wr = abi.RlWireResult()
        for k in ("req_status", "desc_first", "n_descriptors"):
            setattr(wr, k, abi.ptr(wire.get(k)))
        r = v = None
        if out is not None:
            r = abi.RlRequestResult()
            for k in out:
                setattr(r, k, abi.ptr(out[k]))
            if desc_cap is None:
                desc_cap = min([len(a) for k, a in out.items() if k != "stats"] or [0])
        wr.desc_cap = int(desc_cap or 0)
        if verdict is not None:
            v = abi.RlRequestVerdict()
            for k in verdict:
                setattr(v, k, abi.ptr(verdict[k]))
        opts = abi.RL_VERDICT_OPT_GLOBAL_SHADOW if global_shadow else 0
        self._check(self.L.rl_do_limit_wire_async(self.ctx, C.byref(wb.struct), C.byref(wr),
                                                   C.byref(r) if r is not None else None, opts,
                                                   C.byref(v) if v is not None else None))
        return wr, r, v

    def enable_override_rules(self, first_rule: int, capacity: int, key_bytes: int = 0) -> None:
        """rl_override_rules_enable: from now on the wire paths answer messages
        whose descriptors carry a ``limit`` override on the device, their stats
        keys interned there to the rule ids first_rule, first_rule + 1, ...
        (at most ``capacity`` of them; ``key_bytes``: room for their bytes, 0 =
        64 per key). Once per Backend."""
        cfg = abi.RlOverrideRulesConfig()
        cfg.first_rule, cfg.capacity, cfg.key_bytes = int(first_rule), int(capacity), int(key_bytes)
        self._check(self.L.rl_override_rules_enable(self.ctx, C.byref(cfg)))

    def override_rules_info(self) -> dict:
        """rl_override_rules_info_get, after every submitted batch."""
        info = abi.RlOverrideRulesInfo()
        self._check(self.L.rl_override_rules_info_get(self.ctx, C.byref(info)))
        return {f: int(getattr(info, f)) for f, _ in info._fields_ if f != "reserved"}

    def override_rule_keys(self, from_rule: Optional[int] = None, n: Optional[int] = None) -> List[bytes]:
        """rl_override_rule_keys: the stats keys (bytes) of the override rule
        ids [from_rule, from_rule + n); by default all that were handed out."""
        if from_rule is None or n is None:
            info = self.override_rules_info()
            if from_rule is None:
                from_rule = info["first_rule"]
            if n is None:
                n = info["first_rule"] + info["rules"] - from_rule
        off = np.zeros(n + 1, np.uint32)
        need = C.c_uint64(0)
        rc = self.L.rl_override_rule_keys(self.ctx, from_rule, n, None, 0, abi.ptr(off), C.byref(need))
        if rc == abi.RL_OK:  # (no bytes at all)
            return [b""] * n
        if rc != abi.RL_E_CAPACITY:
            self._check(rc)
        buf = np.zeros(max(need.value, 1), np.uint8)
        self._check(self.L.rl_override_rule_keys(self.ctx, from_rule, n, abi.ptr(buf), need.value, abi.ptr(off),
                                                 C.byref(need)))
        raw = buf.tobytes()
        return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]

    @staticmethod
    def response_bound(n_requests: int, n_descriptors: int, header_keys=None) -> int:
        """rl_response_bound: no batch of that shape serializes to more bytes."""
        f, _keep = abi.make_response_format(header_keys)
        return int(lib().rl_response_bound(n_requests, n_descriptors, C.byref(f)))

    def do_limit_wire_respond_async(self, wb: WireRequests, wire: dict, out: Optional[dict], verdict: Optional[dict],
                                    resp: dict, header_keys=None, global_shadow: bool = False,
                                    desc_cap: Optional[int] = None, bytes_cap: Optional[int] = None):
        """rl_do_limit_wire_respond_async: do_limit_wire_async plus the serialized
        RateLimitResponse payloads. ``resp``: ``bytes`` (uint8, from a PinnedArena;
        ``bytes_cap`` defaults to its length) and ``resp_off`` (uint32 x (n + 1));
        ``header_keys``: the (limit, remaining, reset) header names as bytes, or
        None for no headers. ``out`` and ``verdict`` may both be None."""
        wr = abi.RlWireResult()
        for k in ("req_status", "desc_first", "n_descriptors"):
            setattr(wr, k, abi.ptr(wire.get(k)))
        r = v = None
        if out is not None:
            r = abi.RlRequestResult()
            for k in out:
                setattr(r, k, abi.ptr(out[k]))
            if desc_cap is None:
                desc_cap = min([len(a) for k, a in out.items() if k != "stats"] or [0])
        wr.desc_cap = int(desc_cap or 0)
        if verdict is not None:
            v = abi.RlRequestVerdict()
            for k in verdict:
                setattr(v, k, abi.ptr(verdict[k]))
        f, keep = abi.make_response_format(header_keys)
        rb = abi.RlResponseBatch()
        rb.bytes, rb.resp_off = abi.ptr(resp.get("bytes")), abi.ptr(resp.get("resp_off"))
        rb.bytes_cap = len(resp["bytes"]) if bytes_cap is None else int(bytes_cap)
        opts = abi.RL_VERDICT_OPT_GLOBAL_SHADOW if global_shadow else 0
        self._check(self.L.rl_do_limit_wire_respond_async(self.ctx, C.byref(wb.struct), C.byref(wr),
                                                           C.byref(r) if r is not None else None, opts,
                                                           C.byref(v) if v is not None else None, C.byref(f),
                                                           C.byref(rb)))
        return wr, r, v, rb, keep

    @staticmethod
    def response_serialize(desc_first, req_status, res: dict, verdict: dict, header_keys=None):
        """rl_response_serialize (host code): the per-descriptor answers ``res``
        and the per-request ``verdict`` arrays -> (bytes, resp_off), request q's
        serialized RateLimitResponse being bytes[resp_off[q]:resp_off[q + 1]]."""
        L = lib()
        first = np.ascontiguousarray(desc_first, np.uint32)
        nq = len(first) - 1
        st = None if req_status is None else np.ascontiguousarray(req_status, np.uint8)
        keep = []
        r = abi.RlRequestResult()
        for k, dt in abi.REQUEST_RESULT_DTYPES.items():
            if res.get(k) is not None:
                keep.append(np.ascontiguousarray(res[k], dt))
                setattr(r, k, abi.ptr(keep[-1]))
        v = abi.RlRequestVerdict()
        for k, dt in abi.REQUEST_VERDICT_DTYPES.items():
            if verdict.get(k) is not None:
                keep.append(np.ascontiguousarray(verdict[k], dt))
                setattr(v, k, abi.ptr(keep[-1]))
        f, fkeep = abi.make_response_format(header_keys)
        off = np.zeros(nq + 1, np.uint32)
        need = C.c_uint64(0)
        rc = L.rl_response_serialize(nq, abi.ptr(first), abi.ptr(st), C.byref(r), C.byref(v), C.byref(f), None, 0,
                                     abi.ptr(off), C.byref(need))
        if rc not in (abi.RL_OK, abi.RL_E_CAPACITY):
            raise RedisError("rl_response_serialize: malformed input [%s]" % abi.STATUS_NAMES.get(rc, rc), rc)
        out = np.zeros(max(int(need.value), 1), np.uint8)
        if rc:
            rc = L.rl_response_serialize(nq, abi.ptr(first), abi.ptr(st), C.byref(r), C.byref(v), C.byref(f),
                                         abi.ptr(out), int(need.value), abi.ptr(off), C.byref(need))
            if rc:
                raise RedisError("rl_response_serialize failed [%s]" % abi.STATUS_NAMES.get(rc, rc), rc)
        return out[:int(need.value)], off

    def debug_respond(self, n_requests, req_idx, answers: dict, header_keys=None, global_shadow: bool = False,
                      req_status=None, bytes_cap: Optional[int] = None, out_bytes: Optional[np.ndarray] = None):
        """rl_debug_respond: the device verdict and the device serializer on explicit
        per-descriptor answers (``answers``: code, limit_remaining, reset_s, match,
        requests_per_unit, unit) -> (bytes, resp_off)."""
        req = np.ascontiguousarray(req_idx, np.uint32)
        st = None if req_status is None else np.ascontiguousarray(req_status, np.uint8)
        keep = []
        r = abi.RlRequestResult()
        for k, dt in abi.REQUEST_RESULT_DTYPES.items():
            if answers.get(k) is not None:
                keep.append(np.ascontiguousarray(answers[k], dt))
                setattr(r, k, abi.ptr(keep[-1]))
        f, fkeep = abi.make_response_format(header_keys)
        if bytes_cap is None:
            bytes_cap = self.response_bound(n_requests, len(req), header_keys)
        out = np.zeros(max(bytes_cap, 1), np.uint8) if out_bytes is None else out_bytes
        off = np.zeros(n_requests + 1, np.uint32)
        rb = abi.RlResponseBatch()
        rb.bytes, rb.bytes_cap, rb.resp_off = abi.ptr(out), bytes_cap, abi.ptr(off)
        opts = abi.RL_VERDICT_OPT_GLOBAL_SHADOW if global_shadow else 0
        self._check(self.L.rl_debug_respond(self.ctx, n_requests, len(req), abi.ptr(req), abi.ptr(st), C.byref(r), opts,
                                             C.byref(f), C.byref(rb)))
        return out, off

    def debug_verdict(self, n_requests, req_idx, match, code, limit_remaining, reset_s, requests_per_unit,
                      global_shadow: bool = False) -> dict:
        """rl_debug_verdict: the device verdict alone on explicit per-descriptor answers."""
        a = [np.ascontiguousarray(x, dt) for x, dt in
             ((req_idx, np.uint32), (match, np.uint8), (code, np.uint8), (limit_remaining, np.uint32),
              (reset_s, np.uint32), (requests_per_unit, np.uint32))]
        ver = {k: np.zeros(max(n_requests, 1), dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
        gs = np.zeros(1, np.uint64)
        v = abi.RlRequestVerdict()
        for k in ver:
            setattr(v, k, abi.ptr(ver[k]))
        v.global_shadow = abi.ptr(gs)
        opts = abi.RL_VERDICT_OPT_GLOBAL_SHADOW if global_shadow else 0
        self._check(self.L.rl_debug_verdict(self.ctx, n_requests, len(a[0]), *[abi.ptr(x) for x in a], opts,
                                             C.byref(v)))
        res = {k: x[:n_requests] for k, x in ver.items()}
        res["global_shadow"] = int(gs[0])
        return res

    def profile(self, enable: bool, every: int = 1):
        """Time every ``every``-th batch's stages with HIP events (rl_profile)."""
        self._check(self.L.rl_profile(self.ctx, max(int(every), 1) if enable else 0))

    def profile_read(self):
        """-> ({prepare, sort, segment, table, finish} summed ms over the timed batches, and
        table_kernel: k_table's device-clock run time averaged per batch}, batches timed);
        resets the sums."""
        ms = (C.c_double * len(PROFILE_FIELDS))()
        nb = C.c_uint64(0)
        self._check(self.L.rl_profile_read(self.ctx, ms, len(PROFILE_FIELDS), C.byref(nb)))
        return dict(zip(PROFILE_FIELDS, list(ms))), nb.value

    def synchronize(self):
        self._check(self.L.rl_synchronize(self.ctx))

    def restore(self, stems: Sequence[bytes], units, nows, counts, lc=None):
        from .packing import arrays_from_lists
        n = len(stems)
        a = arrays_from_lists(list(stems), [], [0] * n, units, [0] * n, [0] * n, [0] * n, [0] * n)
        nowa = np.asarray(nows, np.int64)
        cnt = np.asarray(counts, np.uint32)
        lca = np.asarray(lc if lc is not None else [0] * n, np.uint8)
        rb = abi.RlRestoreBatch()
        rb.n = n
        rb.stem_bytes, rb.stem_off, rb.unit = abi.ptr(a["stem_bytes"]), abi.ptr(a["stem_off"]), abi.ptr(a["unit"])
        rb.now, rb.count, rb.lc = abi.ptr(nowa), abi.ptr(cnt), abi.ptr(lca)
        self._check(self.L.rl_restore(self.ctx, C.byref(rb)))

    def sweep(self, now: int) -> int:
        ev = C.c_uint64(0)
        self._check(self.L.rl_sweep(self.ctx, now, C.byref(ev)))
        return ev.value

    def table_info(self, shard=None) -> dict:
        """Table counters summed over shards (or of one shard)."""
        info = abi.RlTableInfo()
        if shard is None:
            self._check(self.L.rl_table_info_get(self.ctx, C.byref(info)))
        else:
            self._check(self.L.rl_table_info_shard(self.ctx, shard, C.byref(info)))
        return {f: getattr(info, f) for f, _ in abi.RlTableInfo._fields_}

    def local_cache_info(self, now: int) -> dict:
        """localCacheStats gauges (src/limiter/local_cache_stats.go:20-43)."""
        info = abi.RlLocalCacheInfo()
        self._check(self.L.rl_local_cache_info_get(self.ctx, now, C.byref(info)))
        return {f: getattr(info, f) for f, _ in abi.RlLocalCacheInfo._fields_}

    def snapshot(self) -> np.ndarray:
        """Exact table image (counters, local cache, arena, time floor) as host bytes."""
        nb = C.c_uint64(0)
        self._check(self.L.rl_snapshot_size(self.ctx, C.byref(nb)))
        buf = np.empty(nb.value, np.uint8)
        self._check(self.L.rl_snapshot_save(self.ctx, abi.ptr(buf), nb.value))
        return buf

    def load_snapshot(self, buf: np.ndarray) -> None:
        buf = np.ascontiguousarray(buf, np.uint8)
        self._check(self.L.rl_snapshot_load(self.ctx, abi.ptr(buf), buf.size))

    def resize(self, table_slots: int) -> dict:
        """rl_resize: every shard's table becomes table_slots slots (a power of two;
        larger, smaller or equal: equal drops the tombstones), every live key placed
        in it on the device, the ctx and all its other state kept. Returns the
        rl_resize_info fields. Raises RedisError with the call's status
        (RL_E_TABLE_FULL: the keys do not fit) and leaves the table as it was."""
        info = abi.RlResizeInfo()
        self._check(self.L.rl_resize(self.ctx, table_slots, C.byref(info)))
        self.cfg.table_slots = table_slots
        return {f: getattr(info, f) for f, _ in abi.RlResizeInfo._fields_ if f != "reserved"}

    def resize_history(self, history_entries: int) -> dict:
        """rl_resize_history: every shard's history log is rebuilt at history_entries
        (rounded as at creation; larger, smaller or equal: equal drops every entry no
        live chain reaches), the live chains copied on the device, no answer
        changed. Returns the rl_history_resize_info fields. Raises RedisError with
        the call's status (RL_E_CAPACITY: the live chains do not fit) and leaves
        the log as it was."""
        info = abi.RlHistoryResizeInfo()
        self._check(self.L.rl_resize_history(self.ctx, history_entries, C.byref(info)))
        self.cfg.history_entries = info.entries_after // self.n_shards()
        return {f: getattr(info, f) for f, _ in abi.RlHistoryResizeInfo._fields_ if f != "reserved"}

    def resize_arena(self, arena_bytes: int) -> None:
        """rl_resize_arena: every shard's long-stem arena (and the sweep's spare one)
        becomes arena_bytes, the used bytes copied on the device. Raises RedisError
        (RL_E_ARENA_FULL: more bytes are in use; sweep first) and changes nothing."""
        self._check(self.L.rl_resize_arena(self.ctx, arena_bytes))
        self.cfg.arena_bytes = arena_bytes

    # ---- export / import of live counters (resize, reshard, re-key)
    def n_shards(self) -> int:
        return max(int(self.cfg.n_shards), 1)

    def export_range(self, shard: int, slot_begin: int, slot_end: int, bufs: Optional[dict] = None):
        """rl_export_range -> (records, info). records: numpy arrays stem_bytes,
        stem_off (n + 1) and unit / flags / ws / count / expire / lc (n each), one
        record per (stem, unit, window), a key's records contiguous and oldest
        first; views of `bufs` (a dict this call fills and grows: pass the same one
        to reuse the buffers, then copy what must outlive the next call). On
        RL_E_CAPACITY the buffers grow to what info says and the range is retried once."""
        bufs = bufs if bufs is not None else {}
        info = abi.RlExportInfo()
        for attempt in (0, 1):
            cap = len(bufs["ws"]) if bufs else 0
            if not bufs:
                self._export_alloc(bufs, 4096, 1 << 18)
                cap = 4096
            r = abi.RlRecords()
            r.n, r.stem_cap = cap, len(bufs["stem_bytes"])
            for k in ("stem_bytes", "stem_off") + tuple(abi.RECORD_DTYPES):
                setattr(r, k, abi.ptr(bufs[k]))
            rc = self.L.rl_export_range(self.ctx, shard, slot_begin, slot_end, C.byref(r), C.byref(info))
            if rc == abi.RL_E_CAPACITY and attempt == 0 and info.stem_bytes < 1 << 32:
                self._export_alloc(bufs, max(cap, info.records), max(len(bufs["stem_bytes"]), info.stem_bytes))
                continue
            self._check(rc)
            break
        n = r.n
        rec = {k: bufs[k][:n] for k in abi.RECORD_DTYPES}
        rec["stem_off"] = bufs["stem_off"][:n + 1]
        rec["stem_bytes"] = bufs["stem_bytes"][:int(bufs["stem_off"][n])]
        return rec, {f: getattr(info, f) for f, _ in abi.RlExportInfo._fields_}

    @staticmethod
    def _export_alloc(bufs: dict, n: int, stem_cap: int) -> None:
        bufs["stem_bytes"] = np.zeros(max(int(stem_cap), 1), np.uint8)
        bufs["stem_off"] = np.zeros(int(n) + 1, np.uint32)
        for k, dt in abi.RECORD_DTYPES.items():
            bufs[k] = np.zeros(max(int(n), 1), dt)

    def export_records(self, chunk_slots: int = 1 << 20):
        """The whole table as records: iterates every shard in ranges of
        chunk_slots slots and yields one dict per range: export_range's arrays
        (fresh copies) plus "shard" and "info" (that range's rl_export_info)."""
        bufs = {}
        for shard in range(self.n_shards()):
            lo, slots = 0, None
            while slots is None or lo < slots:
                rec, info = self.export_range(shard, lo, lo + chunk_slots, bufs)
                slots = info["shard_slots"]
                lo += chunk_slots
                out = {k: v.copy() for k, v in rec.items()}
                out["shard"], out["info"] = shard, info
                yield out

    def import_records(self, rec: dict) -> int:
        """rl_import of export_range's arrays, split at any record boundary into
        calls of at most max_batch records and max_stem_bytes stem bytes. Returns the calls made."""
        n = len(rec["ws"])
        max_n = int(self.cfg.max_batch) or 1 << 20
        max_b = int(self.cfg.max_stem_bytes) or 128 * max_n
        off = np.ascontiguousarray(rec["stem_off"], np.uint32)
        stems = np.ascontiguousarray(rec["stem_bytes"], np.uint8)
        cols = {k: np.ascontiguousarray(rec[k], dt) for k, dt in abi.RECORD_DTYPES.items()}
        calls, lo = 0, 0
        while lo < n:
            hi = min(n, lo + max_n)
            if int(off[hi]) - int(off[lo]) > max_b:  # the most records whose stems fit
                hi = max(lo + 1, int(np.searchsorted(off, int(off[lo]) + max_b, side="right")) - 1)
            r = abi.RlRecords()
            r.n = hi - lo
            sub_off = np.ascontiguousarray(off[lo:hi + 1] - off[lo])
            sub_stem = stems[int(off[lo]):int(off[hi])]
            sub = {k: v[lo:hi] for k, v in cols.items()}
            r.stem_bytes, r.stem_off = abi.ptr(sub_stem), abi.ptr(sub_off)
            for k, v in sub.items():
                setattr(r, k, abi.ptr(v))
            self._check(self.L.rl_import(self.ctx, C.byref(r)))
            calls += 1
            lo = hi
        return calls

    # ---- keyed read of counters (Redis GET + TTL, no hit counted)
    def lookup(self, stems: Sequence[bytes], units, nows) -> dict:
        """rl_lookup of the keys (stems[i], units[i]) read at the clocks nows[i], in
        calls of at most max_batch keys and max_stem_bytes stem bytes. Returns
        numpy arrays status / found / count / expire / lc, one entry per key
        (abi.KEY_STATE_DTYPES); a key's failure is its status, a failed call raises."""
        n = len(stems)
        max_n = int(self.cfg.max_batch) or 1 << 20
        max_b = int(self.cfg.max_stem_bytes) or 128 * max_n
        unit = np.ascontiguousarray(units, np.uint8).reshape(-1)
        now = np.ascontiguousarray(nows, np.int64).reshape(-1)
        if len(unit) != n or len(now) != n:
            raise ValueError("lookup: stems, units and nows must have one entry per key")
        off = np.zeros(n + 1, np.int64)
        if n:
            off[1:] = np.cumsum([len(s) for s in stems], dtype=np.int64)
        blob = np.frombuffer(b"".join(stems), np.uint8) if n and off[n] else np.zeros(0, np.uint8)
        out = {k: np.zeros(n, dt) for k, dt in abi.KEY_STATE_DTYPES.items()}
        lo = 0
        while lo < n:
            hi = min(n, lo + max_n)
            if int(off[hi]) - int(off[lo]) > max_b:  # the most keys whose stems fit (one alone: the call says so)
                hi = max(lo + 1, int(np.searchsorted(off, int(off[lo]) + max_b, side="right")) - 1)
            sub_off = np.ascontiguousarray(off[lo:hi + 1] - off[lo], np.uint32)
            sub_stem = np.ascontiguousarray(blob[int(off[lo]):int(off[hi])])
            if sub_stem.size == 0:
                sub_stem = np.zeros(1, np.uint8)
            k = abi.RlKeys()
            k.n = hi - lo
            k.stem_bytes, k.stem_off = abi.ptr(sub_stem), abi.ptr(sub_off)
            sub_unit, sub_now = unit[lo:hi], now[lo:hi]
            k.unit, k.now = abi.ptr(sub_unit), abi.ptr(sub_now)
            res = {f: np.zeros(hi - lo, dt) for f, dt in abi.KEY_STATE_DTYPES.items()}
            s = abi.RlKeyState()
            for f, v in res.items():
                setattr(s, f, abi.ptr(v))
            self._check(self.L.rl_lookup(self.ctx, C.byref(k), C.byref(s)))
            for f, v in res.items():
                out[f][lo:hi] = v
            lo = hi
        return out

    # ---- deletion by stem or stem prefix (Redis DEL, SCAN MATCH + DEL)
    def forget(self, stems: Sequence[bytes], prefix: bool = False, dry_run: bool = False) -> dict:
        """rl_forget of the stems (prefix=True: of every stem that begins with one
        of them; at most 64 prefixes of 4096 bytes in all, one call). A stem goes
        whole: every unit slot, window, history chain and local-cache entry.
        Keyed stems go in calls of at most max_batch stems and max_stem_bytes
        bytes. dry_run: select and count only. Returns "removed" (numpy uint32, the
        slots removed per entry; a prefix's: those not counted under an earlier
        one) and the rl_forget_info fields summed over the calls. Raises
        RedisError with the call's status on failure."""
        n = len(stems)
        flags = (abi.RL_FORGET_PREFIX if prefix else 0) | (abi.RL_FORGET_DRY_RUN if dry_run else 0)
        max_n = n if prefix else int(self.cfg.max_batch) or 1 << 20
        max_b = 1 << 32 if prefix else int(self.cfg.max_stem_bytes) or 128 * max_n
        off = np.zeros(n + 1, np.int64)
        if n:
            off[1:] = np.cumsum([len(s) for s in stems], dtype=np.int64)
        blob = np.frombuffer(b"".join(stems), np.uint8) if n and off[n] else np.zeros(0, np.uint8)
        out = {f: 0 for f, _ in abi.RlForgetInfo._fields_}
        out["removed"] = np.zeros(n, np.uint32)
        lo = 0
        while lo < n:
            hi = min(n, lo + max_n)
            if int(off[hi]) - int(off[lo]) > max_b:  # the most stems whose bytes fit (one alone: the call says so)
                hi = max(lo + 1, int(np.searchsorted(off, int(off[lo]) + max_b, side="right")) - 1)
            sub_off = np.ascontiguousarray(off[lo:hi + 1] - off[lo], np.uint32)
            sub_stem = np.ascontiguousarray(blob[int(off[lo]):int(off[hi])])
            if sub_stem.size == 0:
                sub_stem = np.zeros(1, np.uint8)
            s = abi.RlStems()
            s.n, s.flags = hi - lo, flags
            s.stem_bytes, s.stem_off = abi.ptr(sub_stem), abi.ptr(sub_off)
            removed = np.zeros(hi - lo, np.uint32)
            info = abi.RlForgetInfo()
            self._check(self.L.rl_forget(self.ctx, C.byref(s), abi.ptr(removed), C.byref(info)))
            out["removed"][lo:hi] = removed
            for f, _ in abi.RlForgetInfo._fields_:
                out[f] += int(getattr(info, f))
            lo = hi
        return out

    # ---- listing by stem prefix, page by page (Redis SCAN MATCH + GET / TTL)
    def _scan_query(self, prefixes, units, now, newest):
        """-> (rl_scan_query, the arrays it points to)."""
        prefixes = [bytes(p) for p in prefixes]
        n = len(prefixes)
        off = np.zeros(n + 1, np.uint32)
        if n:
            off[1:] = np.cumsum([len(p) for p in prefixes], dtype=np.int64)
        blob = np.frombuffer(b"".join(prefixes) or b"\0", np.uint8).copy()
        q = abi.RlScanQuery()
        q.n_prefixes = n
        q.flags = (abi.RL_SCAN_NEWEST if newest else 0) | (abi.RL_SCAN_LIVE if now is not None else 0)
        q.prefix_bytes, q.prefix_off = abi.ptr(blob), abi.ptr(off)
        q.now = int(now) if now is not None else 0
        q.unit_mask = 0
        for u in (units if units is not None else ()):
            q.unit_mask |= 1 << int(u)
        return q, (blob, off)

    def scan(self, prefixes: Sequence[bytes] = (), units=None, now: Optional[int] = None, newest: bool = False,
             page_records: int = 1 << 16, page_stem_bytes: Optional[int] = None):
        """rl_scan over every shard, page by page: a generator of (records, info,
        by_prefix). records: export_range's arrays (fresh ones per page) of the
        keys whose stem begins with one of `prefixes` (none: every key), a key's
        records contiguous and oldest first. units: the rl_unit values to select
        (None: every unit); now: only records live at that clock (RL_SCAN_LIVE);
        newest: only each key's newest window. info: rl_scan_info as a dict plus
        "shard" and "cursor" (the (shard, slot) the next page starts at);
        by_prefix: numpy uint64 [max(len(prefixes), 1), 3] of keys, records,
        hits. A page holds at most page_records records and page_stem_bytes stem
        bytes (default 64 per record); where one tile alone needs more
        (RL_E_CAPACITY) the buffers grow to what info asks and the page is retried
        once. Raises RedisError with the call's status otherwise."""
        q, keep = self._scan_query(prefixes, units, now, newest)
        nbins = max(int(q.n_prefixes), 1)
        cur = abi.RlScanCursor()
        n_cap = int(page_records)
        stem_cap = int(page_stem_bytes) if page_stem_bytes is not None else 64 * max(n_cap, 1)
        n_shards = self.n_shards()
        while cur.shard < n_shards:
            info = abi.RlScanInfo()
            byp = np.zeros((nbins, 3), np.uint64)
            shard = int(cur.shard)
            for attempt in (0, 1):
                bufs = {}
                self._export_alloc(bufs, n_cap, stem_cap)
                r = abi.RlRecords()
                r.n, r.stem_cap = n_cap, stem_cap
                for k in ("stem_bytes", "stem_off") + tuple(abi.RECORD_DTYPES):
                    setattr(r, k, abi.ptr(bufs[k]))
                rc = self.L.rl_scan(self.ctx, C.byref(q), C.byref(cur), C.byref(r), abi.ptr(byp), C.byref(info))
                if rc == abi.RL_E_CAPACITY and attempt == 0 and (info.need_records or info.need_stem_bytes):
                    n_cap = max(n_cap, int(info.need_records))
                    stem_cap = max(stem_cap, int(info.need_stem_bytes))
                    continue
                self._check(rc)
                break
            n = r.n
            rec = {k: bufs[k][:n] for k in abi.RECORD_DTYPES}
            rec["stem_off"] = bufs["stem_off"][:n + 1]
            rec["stem_bytes"] = bufs["stem_bytes"][:int(bufs["stem_off"][n])]
            d = {f: getattr(info, f) for f, _ in abi.RlScanInfo._fields_}
            d["shard"], d["cursor"] = shard, (int(cur.shard), int(cur.slot))
            yield rec, d, byp
        del keep

    def count_keys(self, prefixes: Sequence[bytes] = (), units=None, now: Optional[int] = None,
                   newest: bool = False) -> dict:
        """rl_scan's count-only form summed over the shards: the rl_scan_info sums
        (slots_scanned, keys, records, stem_bytes, chains_lost) and "by_prefix"
        (numpy uint64 [max(len(prefixes), 1), 3]: keys, records, hits). Nothing
        but the sums crosses to the host."""
        q, keep = self._scan_query(prefixes, units, now, newest)
        nbins = max(int(q.n_prefixes), 1)
        out = {f: 0 for f in ("slots_scanned", "keys", "records", "stem_bytes", "chains_lost")}
        out["by_prefix"] = np.zeros((nbins, 3), np.uint64)
        cur = abi.RlScanCursor()
        n_shards = self.n_shards()
        while cur.shard < n_shards:
            info = abi.RlScanInfo()
            byp = np.zeros((nbins, 3), np.uint64)
            self._check(self.L.rl_scan(self.ctx, C.byref(q), C.byref(cur), None, abi.ptr(byp), C.byref(info)))
            for f in ("slots_scanned", "keys", "records", "stem_bytes", "chains_lost"):
                out[f] += int(getattr(info, f))
            out["by_prefix"] += byp
        del keep
        return out

    # ---- the busiest / the currently blocked keys (redis-cli --hotkeys, SCAN with a filter)
    def hot_keys(self, now: int, k: int, min_count: int = 0, units=None, blocked: bool = False):
        """rl_hot_keys -> (records, info): the k matching records with the largest
        counts in the windows `now` falls in (export_range's arrays; count
        descending, ties by stem bytes, then unit) and rl_hot_info as a dict.
        units: the rl_unit values to select (None: every unit); blocked: only
        keys the local over-limit cache rejects at `now`. The buffers are sized
        from k; on RL_E_CAPACITY (long stems) they grow to what info allows
        (min(k, matched) records of at most 65535 stem bytes) and the call is
        retried once."""
        q = abi.RlHotQuery()
        q.now, q.k, q.min_count = int(now), int(k), int(min_count)
        q.unit_mask = 0
        for u in (units if units is not None else ()):
            q.unit_mask |= 1 << int(u)
        q.flags = abi.RL_HOT_BLOCKED if blocked else 0
        info = abi.RlHotInfo()
        n_cap, stem_cap = int(k), max(1 << 16, 128 * int(k))
        for attempt in (0, 1):
            bufs = {"stem_bytes": np.empty(max(stem_cap, 1), np.uint8), "stem_off": np.zeros(n_cap + 1, np.uint32)}
            for f, dt in abi.RECORD_DTYPES.items():
                bufs[f] = np.zeros(max(n_cap, 1), dt)
            r = abi.RlRecords()
            r.n, r.stem_cap = n_cap, stem_cap
            for f, v in bufs.items():
                setattr(r, f, abi.ptr(v))
            rc = self.L.rl_hot_keys(self.ctx, C.byref(q), C.byref(r), C.byref(info))
            if rc == abi.RL_E_CAPACITY and attempt == 0:
                n_cap = min(int(k), int(info.matched))
                stem_cap = min(max(n_cap, 1) * 65535, (1 << 32) - 1)
                continue
            self._check(rc)
            break
        n = r.n
        rec = {f: bufs[f][:n] for f in abi.RECORD_DTYPES}
        rec["stem_off"] = bufs["stem_off"][:n + 1]
        rec["stem_bytes"] = bufs["stem_bytes"][:int(bufs["stem_off"][n])]
        return rec, {f: getattr(info, f) for f, _ in abi.RlHotInfo._fields_ if f != "reserved"}

    def debug_keys(self, pb: PackedBatch) -> List[str]:
        cap = int(pb.arrays["stem_off"][-1]) + 24 * pb.n + 1
        buf = np.zeros(cap, np.uint8)
        off = np.zeros(pb.n + 1, np.uint32)
        b = pb.batch_struct()
        self._check(self.L.rl_debug_keys(self.ctx, C.byref(b), abi.ptr(buf), abi.ptr(off), cap))
        return [bytes(buf[off[i]:off[i + 1]]).decode() for i in range(pb.n)]

    def debug_decide(self, before, after, lc_hit, hits, limit, unit, flags, now):
        n = len(before)
        a = [np.ascontiguousarray(x, dt) for x, dt in
             ((before, np.uint32), (after, np.uint32), (lc_hit, np.uint8), (hits, np.uint32), (limit, np.uint32),
              (unit, np.uint8), (flags, np.uint8), (now, np.int64))]
        code = np.zeros(n, np.uint8)
        rem = np.zeros(n, np.uint32)
        reset = np.zeros(n, np.uint32)
        deltas = np.zeros(n * abi.RL_NUM_STATS, np.uint64)
        lc_set = np.zeros(n, np.uint8)
        self._check(self.L.rl_debug_decide(self.ctx, n, *[abi.ptr(x) for x in a], abi.ptr(code), abi.ptr(rem),
                                              abi.ptr(reset), abi.ptr(deltas), abi.ptr(lc_set)))
        return code, rem, reset, deltas.reshape(n, abi.RL_NUM_STATS), lc_set


def migrate(src: Backend, dst: Backend, chunk_slots: int = 1 << 20) -> dict:
    """Move every live counter of src into dst (any table_slots, history_entries,
    hash_seed or shard count): export_records -> import_records. Returns the
    summed rl_export_info (records, stem_bytes, keys, chains_lost; shard_slots
    summed over shards; time_floor the source's). rl_import leaves dst's sweep
    floor alone, so the source's floor is carried over with a sweep of dst at
    that clock once every record is in: a request that src would refuse for its
    clock (RL_E_TIME: the keys it swept may have held that window) is refused by
    dst too, never counted afresh. The sweep evicts nothing src kept (src swept
    at that floor itself) and leaves a higher floor of dst's own as it is.
    Raises RedisError when dst cannot take a record (RL_E_TABLE_FULL /
    RL_E_ARENA_FULL: its status)."""
    total = {"shard_slots": 0, "records": 0, "stem_bytes": 0, "keys": 0, "chains_lost": 0, "time_floor": 0}
    shards = set()
    for rec in src.export_records(chunk_slots):
        info = rec["info"]
        for k in ("records", "stem_bytes", "keys", "chains_lost"):
            total[k] += info[k]
        total["time_floor"] = info["time_floor"]
        if rec["shard"] not in shards:
            shards.add(rec["shard"])
            total["shard_slots"] += info["shard_slots"]
        dst.import_records(rec)
    if total["time_floor"] > 0:
        dst.sweep(total["time_floor"])
    return total


# rl_status of a device-level failure: the GPU or its runtime, not a request
DEVICE_FAILURES = (abi.RL_E_HIP, abi.RL_E_COMM, abi.RL_E_INTERNAL)


class HealthMonitor:
    """The batcher's health monitor (go/src/gpu/cache_impl.go healthMonitor):
    a device-level failure fails the server's health check once, the next
    success marks it OK again — what the Redis pool does on its connections
    (src/redis/driver_impl.go:31-52, server.HealthCheckFail / HealthCheckOK,
    src/server/server.go:47-48). Request-level failures (RL_E_TIME,
    RL_E_INVALID, RL_E_CAPACITY, a full table) leave it as it is. `server`:
    an object with health_check_fail() and health_check_ok() (None: off)."""

    def __init__(self, server=None):
        self.server = server
        self.unhealthy = False

    def observe(self, err):
        if self.server is None:
            return
        if isinstance(err, RedisError) and err.status in DEVICE_FAILURES:
            if not self.unhealthy:
                self.server.health_check_fail()
                self.unhealthy = True
        elif err is None and self.unhealthy:
            self.server.health_check_ok()
            self.unhealthy = False


class GpuRateLimitCache:
    """limiter.RateLimitCache backed by libratelimit_hip.so (BACKEND_TYPE=gpu).
    health_server (GPU_HEALTH_CHECK_DEVICE): the server whose health check a
    device failure fails (HealthMonitor)."""

    def __init__(self, time_source: Optional[TimeSource] = None, near_limit_ratio: float = 0.8,
                 local_cache: bool = False, cache_key_prefix: str = "", per_second: bool = False,
                 expiration_jitter_max_seconds: int = 0, health_server=None, **backend_kw):
        self.time_source = time_source or TimeSource()
        self.prefix = cache_key_prefix
        self.interner = RuleInterner()
        self.health = HealthMonitor(health_server)
        self.backend = Backend(near_limit_ratio, local_cache, per_second, expiration_jitter_max_seconds,
                               **backend_kw)

    def close(self):
        self.backend.close()

    def do_limit(self, ctx, request, limits) -> List[DescriptorStatus]:
        """fixedRateLimitCacheImpl.DoLimit semantics for one request."""
        return self.do_limit_batch([(request, limits, self.time_source.unix_now())])[0]

    def do_limit_batch(self, calls, isolate: bool = False) -> list:
        """Many in-flight DoLimit calls (request, limits, now) as one GPU batch, in arrival order.

        isolate=False: any failure raises RedisError for the whole batch.
        isolate=True: a call holding a descriptor the backend could not answer
        gets a RedisError object in place of its statuses (the batcher panics
        that RPC only, as checkError does per DoLimit, fixed_cache_impl.go:90-95);
        every other call is answered."""
        pb = pack_calls(calls, self.prefix, self.interner)
        try:
            res = self.backend.do_limit_packed(pb, isolate)
        except RedisError as e:
            self.health.observe(e)
            raise
        self.health.observe(None)
        outs = [[DescriptorStatus(OK, None, 0, None) for _ in req.descriptors] for req, _, _ in calls]
        code, rem, rst = res["code"], res["limit_remaining"], res["reset_s"]
        failed = {}
        for j, (c, i) in enumerate(pb.origin):
            lim = calls[c][1][i]
            if isolate and res["status"][j]:
                failed.setdefault(c, int(res["status"][j]))
            outs[c][i] = DescriptorStatus(int(code[j]), lim.limit, int(rem[j]), int(rst[j]))
        for c, st in failed.items():
            outs[c] = RedisError("gpu: descriptor failed [%s]" % abi.STATUS_NAMES.get(st, st))
        st = res["stats"].reshape(-1, abi.RL_NUM_STATS)
        # apply the per-rule deltas to the gostats counters (limit.Stats)
        seen = {}
        for request, limits, _ in calls:
            for lim in limits:
                if lim is not None:
                    seen[lim.stats.key] = lim.stats
        for key, stats in seen.items():
            row = st[self.interner.ids[key]]
            for f, v in zip(abi.STAT_FIELDS, row):
                if v:
                    setattr(stats, f, getattr(stats, f) + int(v))
        return outs

    def peek(self, request, limits, now: Optional[int] = None) -> list:
        """What do_limit would read for this request at `now` (default: the time
        source's), without counting a hit: per descriptor None for a nil limit,
        else KeyState(count, ttl_s, over_limit_cached) of its Redis key — the same
        stems do_limit builds (prefix ‖ domain ‖ entries). Raises RedisError when
        a key cannot be answered (its rl_status)."""
        from .packing import stem_of
        if len(request.descriptors) != len(limits):
            raise AssertionError("len(descriptors) != len(limits)")  # base_limiter.go:47
        now = self.time_source.unix_now() if now is None else int(now)
        where, stems, units = [], [], []
        for i, (d, lim) in enumerate(zip(request.descriptors, limits)):
            if lim is None:
                continue
            where.append(i)
            stems.append(stem_of(self.prefix, request.domain, d.entries))
            units.append(int(lim.limit.unit))
        out = [None] * len(limits)
        if not stems:
            return out
        res = self.backend.lookup(stems, units, [now] * len(stems))
        for j, i in enumerate(where):
            st = int(res["status"][j])
            if st:
                raise RedisError("gpu: key lookup failed [%s]" % abi.STATUS_NAMES.get(st, st), st)
            found = bool(res["found"][j])
            out[i] = KeyState(int(res["count"][j]), int(res["expire"][j]) - now if found else None,
                              bool(res["lc"][j]))
        return out

    def hot_keys(self, k: int, now: Optional[int] = None, min_count: int = 0, units=None,
                 blocked: bool = False) -> list:
        """The k keys with the largest counters in the windows `now` (default: the
        time source's) falls in, busiest first; blocked=True: only the keys the
        local over-limit cache is rejecting at `now`. Stems are the cache's own
        (prefix ‖ domain ‖ entries); the Redis key is stem ‖ decimal(ws)."""
        now = self.time_source.unix_now() if now is None else int(now)
        rec, _ = self.backend.hot_keys(now, k, min_count, units, blocked)
        off, blob = rec["stem_off"], rec["stem_bytes"]
        return [HotKey(bytes(blob[int(off[i]):int(off[i + 1])]), int(rec["unit"][i]), int(rec["ws"][i]),
                       int(rec["count"][i]), int(rec["expire"][i]), int(rec["lc"][i]))
                for i in range(len(rec["ws"]))]

    def forget(self, request, limits=None, dry_run: bool = False) -> dict:
        """Delete the request's keys (Redis DEL of every window of each, in both
        stores, and their local-cache entries): the same stems do_limit and peek
        build (prefix ‖ domain ‖ entries), removed whole, whatever units they were
        counted under. limits (optional): descriptors with a nil limit are left
        out, as do_limit leaves them. Returns Backend.forget's dict, "removed"
        in the order of the descriptors taken."""
        from .packing import stem_of
        if limits is not None and len(request.descriptors) != len(limits):
            raise AssertionError("len(descriptors) != len(limits)")  # base_limiter.go:47
        stems = [stem_of(self.prefix, request.domain, d.entries) for i, d in enumerate(request.descriptors)
                 if limits is None or limits[i] is not None]
        return self.backend.forget(stems, dry_run=dry_run)

    def forget_domain(self, domain: str, dry_run: bool = False) -> dict:
        """Delete every key of a domain: the stems that begin with
        cache_key_prefix ‖ domain ‖ '_' (which also begin the keys of a domain
        named domain ‖ '_' ‖ anything, as a Redis SCAN MATCH would see them)."""
        return self.backend.forget([(self.prefix + domain + "_").encode()], prefix=True, dry_run=dry_run)

    def list_keys(self, domain: str, entries=(), live: bool = True, newest: bool = True) -> list:
        """The keys a domain (or, with entries, a descriptor prefix of it) holds:
        a list of HotKey(stem, unit, ws, count, expire, lc), one per window record,
        a key's records contiguous and oldest first. The stem prefix is
        forget_domain's, cache_key_prefix ‖ domain ‖ '_' (with entries: stem_of's
        stem, which also begins the stems of longer descriptors); live: only
        records whose Redis key exists at the time source's now; newest: only
        each key's newest window."""
        from .packing import stem_of
        prefix = stem_of(self.prefix, domain, entries) if entries else (self.prefix + domain + "_").encode()
        now = self.time_source.unix_now() if live else None
        out = []
        for rec, _, _ in self.backend.scan([prefix], now=now, newest=newest):
            off, blob = rec["stem_off"], rec["stem_bytes"]
            out += [HotKey(bytes(blob[int(off[i]):int(off[i + 1])]), int(rec["unit"][i]), int(rec["ws"][i]),
                           int(rec["count"][i]), int(rec["expire"][i]), int(rec["lc"][i]))
                    for i in range(len(rec["ws"]))]
        return out

    def flush(self):
        """Flush(): nothing is asynchronous on the host path."""
        return None


class RequestVerdict(NamedTuple):
    """One request's answer from should_rate_limit_verdicts."""
    code: int                       # RateLimitResponse.OverallCode
    flags: int                      # abi.RL_VERDICT_*
    headers: Optional[tuple]        # (limit, remaining, reset seconds) of the minimumDescriptor, or None
    statuses: Optional[list]        # [DescriptorStatus], or None when not asked for


class GpuRateLimitService:
    """The service step around DoLimit with the config lookup on the GPU:
    constructLimitsToCheck + DoLimit + shouldRateLimitWorker's statuses
    (src/service/ratelimit.go:104-208) for many requests at once through
    ``rl_do_limit_requests``; should_rate_limit_verdicts also takes the overall
    code, the RateLimit-* header values and global shadow mode from the device
    (``rl_do_limit_requests_verdict``, ratelimit.go:163-209). Config is YAML text as
    ``NewRateLimitConfigImpl`` takes it (src/config/config_impl.go:318-330)."""

    def __init__(self, config_files, near_limit_ratio: float = 0.8, local_cache: bool = False,
                 cache_key_prefix: str = "", per_second: bool = False, global_shadow_mode: bool = False,
                 header_keys=None, device_overrides: bool = False, override_capacity: int = 256, **backend_kw):
        from .config import ConfigTree
        self.interner = RuleInterner()
        self.tree = ConfigTree.from_yaml(config_files, cache_key_prefix, self.interner)
        self.global_shadow_mode = global_shadow_mode
        # the (limit, remaining, reset) header names of should_rate_limit_responses_pipelined's
        # serialized responses (settings HeaderRatelimitLimit / -Remaining / -Reset); None: no headers
        self.header_keys = None if header_keys is None else tuple(
            k.encode() if isinstance(k, str) else bytes(k) for k in header_keys)
        self.backend = Backend(near_limit_ratio, local_cache, per_second, **backend_kw)
        self.backend.load_config(self.tree)
        # device_overrides: the payload paths answer messages with a ``limit`` override on the device
        # (rl_override_rules_enable); their stats keys take the rule ids after the config's, at most
        # override_capacity of them, and their names are fetched when a batch's stats first show a new id
        self.device_overrides = bool(device_overrides)
        self._ov_first = len(self.interner.keys)
        self._ov_capacity = int(override_capacity)
        self._ov_names = []
        if self.device_overrides:
            try:
                self.backend.enable_override_rules(self._ov_first, self._ov_capacity)
            except Exception:
                self.backend.close()
                raise
        self.stats = {}  # stats key -> [6 counters] (the gostats store)
        self.global_shadow_count = 0  # stats.GlobalShadowMode (should_rate_limit_verdicts)

    def close(self):
        self.backend.close()

    def _add_stats(self, deltas, keys=None):
        keys = self.interner.keys if keys is None else keys
        st = deltas.reshape(-1, abi.RL_NUM_STATS)
        for i in np.nonzero(st.any(axis=1))[0]:
            row = self.stats.setdefault(keys[i], [0] * abi.RL_NUM_STATS)
            for j in range(abi.RL_NUM_STATS):
                row[j] += int(st[i, j])

    def _wire_rules(self) -> int:
        """n_rules of a payload batch: the config's rule ids, and the device-interned override ids."""
        if self.device_overrides:
            return self._ov_first + self._ov_capacity
        return max(len(self.interner.keys), 1)

    def _wire_keys(self, stats):
        """The stats keys by rule id for a payload batch's stats rows: the
        config's, then the device-interned override keys, fetched only when a
        non-zero row lies beyond the names already held."""
        if not self.device_overrides:
            return None
        rows = np.nonzero(stats.reshape(-1, abi.RL_NUM_STATS).any(axis=1))[0]
        if len(rows) and int(rows[-1]) >= self._ov_first + len(self._ov_names):
            got = self.backend.override_rule_keys(self._ov_first + len(self._ov_names))
            self._ov_names += [k.decode(errors="surrogateescape") for k in got]
        return self.interner.keys[:self._ov_first] + self._ov_names

    def should_rate_limit_verdicts(self, requests, nows, per_descriptor: bool = True):
        """-> ([RequestVerdict] per request in arrival order, this call's
        global-shadow count). The overall code, the flags and the header triple
        (limit, remaining, reset seconds; None without a minimumDescriptor) come
        from the device; ``statuses`` is the [DescriptorStatus] list when
        ``per_descriptor``, else None: then only per-request bytes and the
        per-rule stats deltas cross PCIe."""
        from .config import pack_requests
        for r in requests:  # checkServiceErr (ratelimit.go:151-152)
            if r.domain == "":
                raise ValueError("rate limit domain must not be empty")
            if not r.descriptors:
                raise ValueError("rate limit descriptor list must not be empty")
        a = pack_requests(requests, nows, self.interner)
        n_rules = max(len(self.interner.keys), 1)
        res = self.backend.do_limit_requests_verdict(a, n_rules, self.global_shadow_mode, per_descriptor)
        return self._verdicts(requests, res, per_descriptor)

    def should_rate_limit_verdicts_pipelined(self, batches, per_descriptor: bool = True):
        """``batches``: a list of (requests, nows). Every batch is submitted
        through ``rl_do_limit_requests_packed_async`` without waiting, then one
        synchronize(). -> what should_rate_limit_verdicts returns for each
        batch, in order."""
        from .config import pack_requests
        for requests, _ in batches:  # checkServiceErr (ratelimit.go:151-152)
            for r in requests:
                if r.domain == "":
                    raise ValueError("rate limit domain must not be empty")
                if not r.descriptors:
                    raise ValueError("rate limit descriptor list must not be empty")
        arena = PinnedArena()
        try:
            flight = []
            for requests, nows in batches:
                a = pack_requests(requests, nows, self.interner)
                n_rules = max(len(self.interner.keys), 1)
                p = self.backend.pack_requests(a, n_rules, arena)
                n, nq = p.n_descriptors, p.n_requests
                out = {}
                if per_descriptor:
                    out = {k: arena.array(n, dt) for k, dt in abi.REQUEST_RESULT_DTYPES.items()}
                out["stats"] = arena.array(n_rules * abi.RL_NUM_STATS, np.uint64)
                ver = {k: arena.array(nq, dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
                ver["global_shadow"] = arena.array(1, np.uint64)
                ver["global_shadow"][0] = 0
                keep = self.backend.do_limit_requests_packed_async(p, out, ver, self.global_shadow_mode)
                flight.append((requests, p, out, ver, keep))
            self.backend.synchronize()
            answers = []
            for requests, p, out, ver, _ in flight:
                res = {k: a[:p.n_descriptors] for k, a in out.items() if k != "stats"}
                res["stats"] = out["stats"][:p.n_rules * abi.RL_NUM_STATS]
                res.update({k: a[:p.n_requests] for k, a in ver.items() if k != "global_shadow"})
                res["global_shadow"] = int(ver["global_shadow"][0])
                answers.append(self._verdicts(requests, res, per_descriptor))
            return answers
        finally:
            if self.backend.ctx:
                try:
                    self.backend.synchronize()  # (a failed flight: nothing may still write into the arena)
                except RedisError:
                    pass
            arena.close()

    def should_rate_limit_payloads_pipelined(self, batches, per_descriptor: bool = True):
        """``batches``: a list of (payloads, nows), the payloads serialized
        RateLimitRequest messages as the gRPC server received them. Every batch
        goes through ``rl_do_limit_wire_async`` unparsed, without waiting, then
        one synchronize(). The messages the device deferred (a descriptor with
        a ``limit`` override unless the service was made with
        ``device_overrides``, or past the packed layout's per-item limits) are
        then resubmitted through ``RequestPacker`` and the packed path, batch by
        batch: they take effect after every batch of this call, in batch order.
        -> per batch what should_rate_limit_verdicts returns, a malformed
        message's entry being a RedisError (that request's alone). As on the
        wire nothing is checked before the device, an empty domain or
        descriptor list is answered like any other request."""
        from .config import RequestPacker, batch_arrays
        arena = PinnedArena()
        packer = None
        try:
            n_rules = self._wire_rules()
            max_batch = int(self.backend.cfg.max_batch)
            flight = []
            for msgs, nows in batches:
                wb = self.backend.wire_batch(msgs, nows, arena, n_rules)
                nq = len(msgs)
                cap = max(min(max_batch, wb.msgs_bytes // 2), 1)  # (a descriptor takes 2 payload bytes at least)
                out = {}
                if per_descriptor:
                    out = {k: arena.array(cap, dt) for k, dt in abi.REQUEST_RESULT_DTYPES.items()}
                out["stats"] = arena.array(n_rules * abi.RL_NUM_STATS, np.uint64)
                ver = {k: arena.array(nq, dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
                ver["global_shadow"] = arena.array(1, np.uint64)
                ver["global_shadow"][0] = 0
                wire = {"req_status": arena.array(nq, np.uint8), "desc_first": arena.array(nq + 1, np.uint32),
                        "n_descriptors": arena.array(1, np.uint32)}
                keep = self.backend.do_limit_wire_async(wb, wire, out, ver, self.global_shadow_mode, cap)
                flight.append((wb, wire, out, ver, keep))
            self.backend.synchronize()
            answers = []
            again = []  # (batch, its deferred messages' indices)
            for b, (wb, wire, out, ver, _) in enumerate(flight):
                nq, n = wb.n_requests, int(wire["n_descriptors"][0])
                res = {k: a[:n] for k, a in out.items() if k != "stats"}
                res["stats"] = out["stats"][:n_rules * abi.RL_NUM_STATS]
                res.update({k: a[:nq] for k, a in ver.items() if k != "global_shadow"})
                res["global_shadow"] = int(ver["global_shadow"][0])
                first = wire["desc_first"][:nq + 1]
                vs, shadow = self._verdicts(first[1:] - first[:-1], res, per_descriptor, self._wire_keys(res["stats"]))
                status = wire["req_status"][:nq]
                for q in np.nonzero(status == abi.RL_WIRE_MALFORMED)[0]:
                    vs[q] = RedisError("gpu: malformed RateLimitRequest", abi.RL_E_INVALID)
                deferred = np.nonzero(status == abi.RL_WIRE_DEFERRED)[0]
                if len(deferred):
                    again.append((b, deferred))
                answers.append([vs, shadow])
            for b, deferred in again:
                msgs, nows = batches[b]
                if packer is None:
                    packer = RequestPacker(len(self.interner.keys))
                rb = packer.pack([msgs[q] for q in deferred], [nows[q] for q in deferred])
                a = batch_arrays(rb)
                nr = max(packer.rules(), 1)
                res = self.backend.do_limit_requests_verdict(a, nr, self.global_shadow_mode, per_descriptor)
                keys = self.interner.keys + [packer.rule_key(i) for i in range(len(self.interner.keys), nr)]
                counts = np.bincount(a["req_idx"], minlength=len(deferred))
                vs, shadow = self._verdicts(counts, res, per_descriptor, keys)
                for q, v in zip(deferred, vs):
                    answers[b][0][q] = v
                answers[b][1] += shadow
            return [tuple(x) for x in answers]
        finally:
            if packer is not None:
                packer.close()
            if self.backend.ctx:
                try:
                    self.backend.synchronize()  # (a failed flight: nothing may still write into the arena)
                except RedisError:
                    pass
            arena.close()

    def should_rate_limit_responses_pipelined(self, batches):
        """``batches``: a list of (payloads, nows) as for
        should_rate_limit_payloads_pipelined. Payload bytes in, payload bytes
        out: every batch goes through ``rl_do_limit_wire_respond_async`` and
        comes back as serialized RateLimitResponse messages, written on the
        device; per-descriptor arrays never cross PCIe. The deferred messages
        are resubmitted through ``RequestPacker`` and the packed path as there
        and serialized on the host (``rl_response_serialize``). -> per batch
        ([response bytes per request], this batch's global-shadow count), a
        malformed message's entry being a RedisError (that request's alone)."""
        from .config import RequestPacker, batch_arrays
        arena = PinnedArena()
        packer = None
        hk = self.header_keys
        try:
            n_rules = self._wire_rules()
            max_batch = int(self.backend.cfg.max_batch)
            flight = []
            for msgs, nows in batches:
                wb = self.backend.wire_batch(msgs, nows, arena, n_rules)
                nq = len(msgs)
                cap = max(min(max_batch, wb.msgs_bytes // 2), 1)  # (a descriptor takes 2 payload bytes at least)
                out = {"stats": arena.array(n_rules * abi.RL_NUM_STATS, np.uint64)}
                ver = {"global_shadow": arena.array(1, np.uint64)}
                ver["global_shadow"][0] = 0
                wire = {"req_status": arena.array(nq, np.uint8)}
                resp = {"bytes": arena.array(self.backend.response_bound(nq, cap, hk), np.uint8),
                        "resp_off": arena.array(nq + 1, np.uint32)}
                keep = self.backend.do_limit_wire_respond_async(wb, wire, out, ver, resp, hk, self.global_shadow_mode,
                                                                cap)  # (out holds the stats alone)
                flight.append((wb, wire, out, ver, resp, keep))
            self.backend.synchronize()
            answers = []
            again = []  # (batch, its deferred messages' indices)
            for b, (wb, wire, out, ver, resp, _) in enumerate(flight):
                nq = wb.n_requests
                st = out["stats"][:n_rules * abi.RL_NUM_STATS]
                self._add_stats(st, self._wire_keys(st))
                shadow = int(ver["global_shadow"][0])
                self.global_shadow_count += shadow
                off = resp["resp_off"][:nq + 1]
                raw = resp["bytes"][:int(off[nq])].tobytes()
                rs = [raw[int(off[q]):int(off[q + 1])] for q in range(nq)]
                status = wire["req_status"][:nq]
                for q in np.nonzero(status == abi.RL_WIRE_MALFORMED)[0]:
                    rs[q] = RedisError("gpu: malformed RateLimitRequest", abi.RL_E_INVALID)
                deferred = np.nonzero(status == abi.RL_WIRE_DEFERRED)[0]
                if len(deferred):
                    again.append((b, deferred))
                answers.append([rs, shadow])
            for b, deferred in again:
                msgs, nows = batches[b]
                if packer is None:
                    packer = RequestPacker(len(self.interner.keys))
                rb = packer.pack([msgs[q] for q in deferred], [nows[q] for q in deferred])
                a = batch_arrays(rb)
                nr = max(packer.rules(), 1)
                res = self.backend.do_limit_requests_verdict(a, nr, self.global_shadow_mode, True)
                keys = self.interner.keys + [packer.rule_key(i) for i in range(len(self.interner.keys), nr)]
                self._add_stats(res["stats"], keys)
                self.global_shadow_count += res["global_shadow"]
                first = np.zeros(len(deferred) + 1, np.uint32)
                np.cumsum(np.bincount(a["req_idx"], minlength=len(deferred)), out=first[1:])
                raw, off = self.backend.response_serialize(first, None, res, res, hk)
                raw = raw.tobytes()
                for i, q in enumerate(deferred):
                    answers[b][0][q] = raw[int(off[i]):int(off[i + 1])]
                answers[b][1] += res["global_shadow"]
            return [tuple(x) for x in answers]
        finally:
            if packer is not None:
                packer.close()
            if self.backend.ctx:
                try:
                    self.backend.synchronize()  # (a failed flight: nothing may still write into the arena)
                except RedisError:
                    pass
            arena.close()

    def _verdicts(self, requests, res, per_descriptor, keys=None):
        """One batch's device answers -> should_rate_limit_verdicts' result.
        ``requests``: the requests, or their descriptor counts; ``keys``: the
        stats keys by rule id (default: the config's)."""
        self._add_stats(res["stats"], keys)
        self.global_shadow_count += res["global_shadow"]
        out = []
        d = 0
        for q, r in enumerate(requests):
            sts = None
            if per_descriptor:
                sts = []
                for _ in range(len(r.descriptors) if hasattr(r, "descriptors") else int(r)):
                    if int(res["match"][d]) == abi.RL_MATCH_LIMIT:
                        sts.append(DescriptorStatus(int(res["code"][d]),
                                                    Limit(int(res["requests_per_unit"][d]), int(res["unit"][d])),
                                                    int(res["limit_remaining"][d]), int(res["reset_s"][d])))
                    else:  # nil limit {OK, nil, 0}; unlimited {OK, nil, MaxUint32}
                        sts.append(DescriptorStatus(OK, None, int(res["limit_remaining"][d]), None))
                    d += 1
            headers = None
            if int(res["min_descriptor"][q]) != abi.RL_NO_DESCRIPTOR:
                headers = (int(res["header_limit"][q]), int(res["header_remaining"][q]),
                           int(res["header_reset_s"][q]))
            out.append(RequestVerdict(int(res["overall_code"][q]), int(res["flags"][q]), headers, sts))
        return out, res["global_shadow"]

    def should_rate_limit_batch(self, requests, nows):
        """-> [(overall code, [DescriptorStatus])] per request, arrival order."""
        from .config import pack_requests
        for r in requests:  # checkServiceErr (ratelimit.go:151-152)
            if r.domain == "":
                raise ValueError("rate limit domain must not be empty")
            if not r.descriptors:
                raise ValueError("rate limit descriptor list must not be empty")
        a = pack_requests(requests, nows, self.interner)
        n_rules = max(len(self.interner.keys), 1)
        res = self.backend.do_limit_requests(a, n_rules)
        st = res["stats"].reshape(-1, abi.RL_NUM_STATS)
        for i in np.nonzero(st.any(axis=1))[0]:
            row = self.stats.setdefault(self.interner.keys[i], [0] * abi.RL_NUM_STATS)
            for j in range(abi.RL_NUM_STATS):
                row[j] += int(st[i, j])
        out = []
        d = 0
        OVER = 2
        for r in requests:
            sts = []
            final = OK
            for _ in r.descriptors:
                m = int(res["match"][d])
                if m == abi.RL_MATCH_LIMIT:
                    s_ = DescriptorStatus(int(res["code"][d]),
                                          Limit(int(res["requests_per_unit"][d]), int(res["unit"][d])),
                                          int(res["limit_remaining"][d]), int(res["reset_s"][d]))
                    if s_.code == OVER:
                        final = OVER
                else:  # nil limit {OK, nil, 0}; unlimited {OK, nil, MaxUint32}
                    s_ = DescriptorStatus(OK, None, int(res["limit_remaining"][d]), None)
                sts.append(s_)
                d += 1
            if final == OVER and self.global_shadow_mode:
                final = OK
            out.append((final, sts))
        return out
