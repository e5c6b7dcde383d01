"""The argument errors of the request path, pinned: return code and
rl_last_error text of every refusal the host side of the calls that take raw
requests can give (rl_do_limit_requests[_verdict], ..._packed_async,
rl_do_limit_wire[_respond]_async, rl_debug_verdict / rl_debug_respond, the
override-rules calls, and the section checks of the compact and the prefixed
batch), in a fixed order, on a ctx of one shard and on one of two.

The expected list (tests/golden/own_request_errors.json) was recorded with this
module's case list against the library as it was before the calls' host side
was gathered into rl_requests.hip:

    python tests/test_gpu_request_errors.py --record    # (RL_RECORD_TO=path: written there)

It is never recorded from the code under test. One kind of refusal is left
out: a null ctx. rl_api.hip refuses it before any engine is reached, so it is
no refusal of the host side gathered here, and its text lands in a
thread-local string that rl_last_error(NULL) reads, which no ctx's state can
be compared around. Every case also checks that the
refused call changed nothing rl_table_info_get shows and that a valid call of
the same entry point succeeds right after it. No case needs a device
allocation to fail or a kernel to misbehave; the refusals that arrive at
rl_synchronize are the wire middle stage's capacity checks, each on a
well-formed batch.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pbwire
from oracle import oracle as O
from ratelimit_amd import abi
from ratelimit_amd._lib import lib
from ratelimit_amd.config import ConfigTree, pack_requests
from ratelimit_amd.limiter import Backend, PinnedArena, _config
from ratelimit_amd.packing import RuleInterner, compact_batch, pack_calls, prefixed_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "own_request_errors.json")
T = 1_700_000_040
MAX_BATCH, MAX_REQUESTS, MAX_RULES, STEM_CAP = 64, 16, 8, 4096
YAML = "domain: rq\ndescriptors:\n  - key: k\n    rate_limit:\n      unit: hour\n      requests_per_unit: 100\n"
NQ, N, NE = 2, 4, 4  # the valid batch: two requests of two one-entry descriptors
KEYS = (b"x-ratelimit-limit", b"x-ratelimit-remaining", b"x-ratelimit-reset")


def _requests(nq=NQ, per=2, value="v"):
    return [O.RateLimitRequest("rq", [O.Descriptor([("k", "%s%d_%d" % (value, q, d))]) for d in range(per)], 1)
            for q in range(nq)]


class Ctx(Backend):
    """A ctx of the smallest useful config (max_requests below max_batch), its batches and its pinned outputs."""

    def __init__(self, shards, config=True):
        self.L = lib()
        err = C.create_string_buffer(512)
        self.cfg = _config(0.8, False, False, 0, 1024, MAX_BATCH, MAX_RULES, 0, 1 << 16, STEM_CAP, 7, 0, shards,
                           [0] * shards, 4096)
        self.cfg.max_requests = MAX_REQUESTS
        self.ctx = self.L.rl_create(C.byref(self.cfg), err, 512)
        assert self.ctx, err.value
        self.it = RuleInterner()
        if config:
            self.load_config(ConfigTree.from_yaml([("rq.yaml", YAML)], "", self.it))
        self.arena = PinnedArena()
        self.a = pack_requests(_requests(), [T] * NQ, self.it)
        self.packed = self.pack_requests(self.a, 1, self.arena)
        self.msgs = [pbwire.encode_request(r) for r in _requests()]
        self.wb = Backend.wire_batch(self.msgs, [T] * NQ, self.arena, 1)
        lim = O.new_rate_limit(100, O.HOUR, "rq.k")
        pb = pack_calls([(r, [lim] * 2, T) for r in _requests()], "", RuleInterner())
        pinned = lambda nbytes: self.arena.array(nbytes, np.uint8)  # noqa: E731
        self.compact = compact_batch(pb.arrays, pb.n, pb.n_requests, 1, pinned)
        self.prefixed = prefixed_batch(pb.arrays, pb.n, pb.n_requests, 1, pinned)
        self.res = {k: self.arena.array(MAX_BATCH + 1, dt) for k, dt in abi.REQUEST_RESULT_DTYPES.items()}
        self.res["stats"] = self.arena.array((MAX_RULES + 1) * abi.RL_NUM_STATS, np.uint64)
        self.ver = {k: self.arena.array(MAX_REQUESTS + 1, dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
        self.ver["global_shadow"] = self.arena.array(1, np.uint64)
        self.wire = {"req_status": self.arena.array(MAX_REQUESTS + 1, np.uint8),
                     "desc_first": self.arena.array(MAX_REQUESTS + 2, np.uint32),
                     "n_descriptors": self.arena.array(1, np.uint32)}
        self.resp = {"bytes": self.arena.array(1 << 14, np.uint8), "resp_off": self.arena.array(MAX_REQUESTS + 2, np.uint32)}
        self.plain = {k: np.zeros(MAX_BATCH + 1, dt) for k, dt in abi.RESULT_DTYPES.items()}
        self.ov_enabled = False

    def close(self):
        super().close()
        self.arena.close()


def _struct(cls, arrays, null=()):
    s = cls()
    for k, a in arrays.items():
        setattr(s, k, None if k in null else abi.ptr(a))
    return s


def _copy(s, new_buf=None, **fields):
    """A copy of a ctypes struct with fields changed; new_buf: another buffer for it."""
    c = type(s).from_buffer_copy(s)
    if new_buf is not None:
        c.buf = abi.ptr(new_buf)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def _sync(be, rc):
    """A submitted batch's status: the call's, or rl_synchronize's."""
    return rc if rc else be.L.rl_synchronize(be.ctx)


# ---- rl_do_limit_requests / rl_do_limit_requests_verdict ----------------------------------

def _requests_call(be, verdict=True, no_in=False, no_out=False, no_verdict=False, opts=0, null=(), vnull=(), sizes=None,
                   edit=None, ov=None):
    a = dict(be.a)
    if ov:  # (override arrays of the batch's size)
        a.update(override_flags=np.zeros(N, np.uint8), override_rpu=np.zeros(N, np.uint32),
                 override_unit=np.zeros(N, np.uint8), override_rule=np.zeros(N, np.uint32))
    if edit:
        k, i, v = edit
        a[k] = a[k].copy()
        a[k][i] = v
    b = _struct(abi.RlRequestBatch, {k: a[k] for k in abi.REQUEST_ARRAYS if a[k] is not None}, null)
    b.n_requests, b.n_descriptors, b.n_entries, b.n_rules = sizes or (NQ, N, NE, 1)
    r = _struct(abi.RlRequestResult, be.res)
    v = _struct(abi.RlRequestVerdict, be.ver, vnull)
    pin, pout = (None if no_in else C.byref(b)), (None if no_out else C.byref(r))
    if not verdict:
        return be.L.rl_do_limit_requests(be.ctx, pin, pout)
    return be.L.rl_do_limit_requests_verdict(be.ctx, pin, pout, opts, None if no_verdict else C.byref(v))


REQUEST_NULLS = ("domain_off", "entry_first", "desc_off", "now", "hits", "req_idx", "key_len", "value_len")
REQUESTS_PLAIN = [("null_in", lambda be: _requests_call(be, verdict=False, no_in=True)),
                  ("null_out", lambda be: _requests_call(be, verdict=False, no_out=True))]
REQUESTS = [("null_in", lambda be: _requests_call(be, no_in=True)),
            ("null_verdict", lambda be: _requests_call(be, no_verdict=True)),
            ("verdict_without_overall_code", lambda be: _requests_call(be, vnull=("overall_code",))),
            ("unknown_option", lambda be: _requests_call(be, opts=2)),
            ("descriptors_over_max_batch", lambda be: _requests_call(be, sizes=(NQ, MAX_BATCH + 1, NE, 1))),
            ("requests_over_max_requests", lambda be: _requests_call(be, sizes=(MAX_REQUESTS + 1, N, NE, 1))),
            # (the engines of a ctx of several shards hold n_shards x max_rules rows: the engine's own bound)
            ("rules_over_max_rules", lambda be: _requests_call(be, sizes=(NQ, N, NE, MAX_RULES * be.n_shards() + 1))),
            ("descriptors_without_requests", lambda be: _requests_call(be, sizes=(0, N, NE, 1)))]
REQUESTS += [("null_" + k, lambda be, k=k: _requests_call(be, null=(k,))) for k in REQUEST_NULLS]
REQUESTS += [("override_flags_without_" + k, lambda be, k=k: _requests_call(be, ov=True, null=("override_" + k,)))
             for k in ("rpu", "unit", "rule")]
REQUESTS += [("entry_first_0_not_0", lambda be: _requests_call(be, edit=("entry_first", 0, 1))),
             ("entry_first_end_not_n_entries", lambda be: _requests_call(be, edit=("entry_first", N, NE + 1))),
             ("desc_off_0_not_0", lambda be: _requests_call(be, edit=("desc_off", 0, 1))),
             ("domain_off_0_not_0", lambda be: _requests_call(be, edit=("domain_off", 0, 1))),
             ("null_domain_bytes", lambda be: _requests_call(be, null=("domain_bytes",))),
             ("null_desc_bytes", lambda be: _requests_call(be, null=("desc_bytes",)))]


# ---- the one-buffer batches: sections outside buf or at an odd offset -----------------------

def _section_cases(pr, s, sections, call):
    """sections: {field: its bytes}. Per section: its end just past buf (the offset 4-byte aligned), and an odd offset."""
    B = int(s(pr).buf_bytes)
    out = []
    for k, nbytes in sections.items():
        past = ((B - nbytes) & ~3) + 4 if nbytes else B + 4
        out.append((k + "_outside_buf", lambda be, k=k, past=past: call(be, **{k: past})))
        out.append((k + "_odd_offset", lambda be, k=k: call(be, **{k: int(getattr(s(be), k)) + 1})))
    return out


def _word_edit(be, s, section, word, value):
    """A pinned copy of the batch's buffer with one 32-bit word of a section changed (kept alive by the ctx)."""
    buf = be.arena.like(np.frombuffer(bytes((C.c_uint8 * int(s.buf_bytes)).from_address(s.buf)), np.uint8))
    buf[int(getattr(s, section)):].view(np.uint32)[word] = value
    return buf


def _packed_call(be, no_in=False, out=True, verdict=True, opts=0, edit=None, **fields):
    s = be.packed.struct
    c = _copy(s, _word_edit(be, s, "index", *edit) if edit else None, **fields)
    r, v = _struct(abi.RlRequestResult, be.res), _struct(abi.RlRequestVerdict, be.ver)
    return _sync(be, be.L.rl_do_limit_requests_packed_async(be.ctx, None if no_in else C.byref(c),
                                                            C.byref(r) if out else None, opts,
                                                            C.byref(v) if verdict else None))


def _packed_cases(pr):
    s = pr.packed.struct
    T4 = 4 * ((NQ + abi.RL_REQUESTS_TILE - 1) // abi.RL_REQUESTS_TILE)  # the index's last entry, in words
    sections = {"index": 16 * (T4 // 4 + 1), "req": NQ * 4, "now": NQ * 4, "hits": NQ * 4, "desc": N * 2,
                "key_len": NE * 2, "value_len": NE * 2, "overrides": 0, "domain_bytes": 0, "entry_bytes": 0}
    B = int(s.buf_bytes)
    assert B <= STEM_CAP
    return [("null_in", lambda be: _packed_call(be, no_in=True)),
            ("null_out_and_verdict", lambda be: _packed_call(be, out=False, verdict=False)),
            ("unknown_option", lambda be: _packed_call(be, opts=2)),
            ("descriptors_over_max_batch", lambda be: _packed_call(be, n_descriptors=MAX_BATCH + 1)),
            ("requests_over_max_requests", lambda be: _packed_call(be, n_requests=MAX_REQUESTS + 1)),
            ("rules_over_max_rules", lambda be: _packed_call(be, n_rules=MAX_RULES + 1)),
            ("descriptors_without_requests", lambda be: _packed_call(be, n_requests=0)),
            ("reserved", lambda be: _packed_call(be, reserved=1)),
            ("overrides_over_descriptors", lambda be: _packed_call(be, n_overrides=N + 1)),
            ("null_buf", lambda be: _packed_call(be, buf=None))] + \
        _section_cases(pr, lambda be: be.packed.struct, sections, _packed_call) + \
        [("index_start_not_0", lambda be: _packed_call(be, edit=(0, 1))),
         ("index_start_entries_not_0", lambda be: _packed_call(be, edit=(1, 1))),
         ("index_end_not_n_descriptors", lambda be: _packed_call(be, edit=(T4, N + 1))),
         ("index_end_not_n_entries", lambda be: _packed_call(be, edit=(T4 + 1, NE + 1))),
         ("entry_bytes_over_max_stem_bytes", lambda be: _packed_call(be, edit=(T4 + 3, STEM_CAP + 1))),
         ("domain_bytes_past_buf", lambda be: _packed_call(be, edit=(T4 + 2, B))),
         ("entry_bytes_past_buf", lambda be: _packed_call(be, edit=(T4 + 3, B)))]


def _hostfed_call(be, kind, edit=None, **fields):
    s = (be.compact if kind == "compact" else be.prefixed).struct()
    c = _copy(s, _word_edit(be, s, "stem_off" if kind == "compact" else "index", *edit) if edit else None, **fields)
    r = abi.make_result_struct(be.plain)
    f = be.L.rl_do_limit_compact_async if kind == "compact" else be.L.rl_do_limit_prefixed_async
    return _sync(be, f(be.ctx, C.byref(c), C.byref(r)))


def _compact_cases(pr):
    s = pr.compact.struct()
    call = lambda be, **kw: _hostfed_call(be, "compact", **kw)  # noqa: E731
    sections = {"stem_off": (N + 1) * 4, "limit_idx": N * 2, "req_first": (NQ + 1) * 4, "now": NQ * 4, "hits": NQ * 4,
                "limits": pr.compact.n_limits * 12, "stem_bytes": 0}
    # (stem_off's last word is the stems' size)
    return _section_cases(pr, lambda be: be.compact.struct(), sections, call) + \
        [("stems_over_max_stem_bytes", lambda be: call(be, edit=(N, STEM_CAP + 1))),
         ("stems_past_buf", lambda be: call(be, edit=(N, int(s.buf_bytes))))]


def _prefixed_cases(pr):
    s = pr.prefixed.struct()
    call = lambda be, **kw: _hostfed_call(be, "prefixed", **kw)  # noqa: E731
    T4 = 4 * pr.prefixed.tiles()
    sections = {"index": 16 * (T4 // 4 + 1), "req": NQ * 4, "now": NQ * 4, "hits": NQ * 4, "desc": N * 4,
                "limits": pr.prefixed.n_limits * 12}
    B = int(s.buf_bytes)
    return _section_cases(pr, lambda be: be.prefixed.struct(), sections, call) + \
        [("index_start_not_0", lambda be: call(be, edit=(0, 1))),
         ("index_end_not_n", lambda be: call(be, edit=(T4, N + 1))),
         ("stems_over_max_stem_bytes", lambda be: call(be, edit=(T4 + 3, STEM_CAP + 1))),
         ("prefix_bytes_past_buf", lambda be: call(be, edit=(T4 + 1, B))),
         ("suffix_bytes_past_buf", lambda be: call(be, edit=(T4 + 2, B)))]


# ---- rl_do_limit_wire_async / rl_do_limit_wire_respond_async ---------------------------------

def _wire_call(be, respond=False, wb=None, no_in=False, no_wire=False, wnull=(), out=True, verdict=True, opts=0,
               reserved=0, desc_cap=MAX_BATCH, edit=None, no_resp=False, rnull=(), keys=KEYS, fmt=None, bytes_cap=None,
               pageable=False, **fields):
    s = (wb or be.wb).struct
    c = _copy(s, _word_edit(be, s, "msg_off", *edit) if edit else None, **fields)
    wr = _struct(abi.RlWireResult, be.wire, wnull)
    wr.desc_cap, wr.reserved = desc_cap, reserved
    r, v = _struct(abi.RlRequestResult, be.res), _struct(abi.RlRequestVerdict, be.ver)
    args = [be.ctx, None if no_in else C.byref(c), None if no_wire else C.byref(wr), C.byref(r) if out else None, opts,
            C.byref(v) if verdict else None]
    if not respond:
        return _sync(be, be.L.rl_do_limit_wire_async(*args))
    f, keep = abi.make_response_format(keys)
    for k, x in (fmt or {}).items():
        setattr(f, k, x)
    resp = dict(be.resp, bytes=np.zeros(1 << 14, np.uint8)) if pageable else be.resp
    rb = _struct(abi.RlResponseBatch, resp, rnull)
    rb.bytes_cap = len(resp["bytes"]) if bytes_cap is None else bytes_cap
    return _sync(be, be.L.rl_do_limit_wire_respond_async(*args, C.byref(f), None if no_resp else C.byref(rb)))


def _wire_cases(pr, respond):
    call = lambda be, **kw: _wire_call(be, respond, **kw)  # noqa: E731
    sections = {"msg_off": (NQ + 1) * 4, "now": NQ * 4, "msgs": int(pr.wb.struct.msgs_bytes)}
    big = lambda be: Backend.wire_batch([b""] * (MAX_REQUESTS + 1), [T] * (MAX_REQUESTS + 1), be.arena, 1)  # noqa: E731
    # well-formed batches the middle stage refuses: three descriptors of 2000-byte values; a one-descriptor room
    fat = lambda be: Backend.wire_batch([pbwire.encode_request(r) for r in _requests(1, 3, "w" * 2000)], [T],  # noqa: E731
                                        be.arena, 1)
    cases = [("null_in", lambda be: call(be, no_in=True)),
             ("null_wire", lambda be: call(be, no_wire=True)),
             ("null_req_status", lambda be: call(be, wnull=("req_status",))),
             ("null_outputs", (lambda be: call(be, out=False, verdict=False)) if not respond else None),
             ("unknown_option", lambda be: call(be, opts=2)),
             ("wire_reserved", lambda be: call(be, reserved=1)),
             ("requests_over_max_requests", lambda be: call(be, wb=big(be))),
             ("rules_over_max_rules", lambda be: call(be, n_rules=MAX_RULES + 1)),
             ("null_buf", lambda be: call(be, buf=None)),
             ("msgs_bytes_over_32_bits", lambda be: call(be, msgs_bytes=1 << 32))] + \
        _section_cases(pr, lambda be: be.wb.struct, sections, call) + \
        [("msg_off_start_not_0", lambda be: call(be, edit=(0, 1))),
         ("msg_off_end_not_msgs_bytes", lambda be: call(be, edit=(NQ, int(pr.wb.struct.msgs_bytes) - 1))),
         ("at_synchronize_descriptors_over_desc_cap", lambda be: call(be, desc_cap=N - 1)),
         ("at_synchronize_entry_bytes_over_max_stem_bytes", lambda be: call(be, wb=fat(be)))]
    if respond:
        cases += [("null_resp", lambda be: call(be, no_resp=True)),
                  ("resp_without_bytes", lambda be: call(be, rnull=("bytes",))),
                  ("resp_without_resp_off", lambda be: call(be, rnull=("resp_off",))),
                  ("format_key_over_64", lambda be: call(be, keys=(b"k" * 65, b"r", b"s"))),
                  ("format_null_key_with_length", lambda be: call(be, keys=None, fmt={"limit_key_len": 3})),
                  ("format_reserved", lambda be: call(be, fmt={"reserved": 1})),
                  ("bytes_not_page_locked", lambda be: call(be, pageable=True)),
                  ("at_synchronize_bound_over_bytes_cap", lambda be: call(be, bytes_cap=8))]
    return [c for c in cases if c[1] is not None]


# ---- rl_debug_verdict / rl_debug_respond ------------------------------------------------------

def _answers(n=N):
    a = {k: np.zeros(max(n, 1), dt) for k, dt in abi.REQUEST_RESULT_DTYPES.items()}
    a["code"][:] = 1
    a["match"][:] = abi.RL_MATCH_LIMIT
    a["requests_per_unit"][:] = 100
    a["unit"][:] = 3
    return a


def _debug_verdict(be, nq=NQ, n=N, req=(0, 0, 1, 1), no_verdict=False, vnull=(), opts=0, null=()):
    a = _answers(n)
    req = np.array(list(req) + [0] * max(n - len(req), 0), np.uint32)
    cols = {"req_idx": req, "match": a["match"], "code": a["code"], "limit_remaining": a["limit_remaining"],
            "reset_s": a["reset_s"], "requests_per_unit": a["requests_per_unit"]}
    v = _struct(abi.RlRequestVerdict, be.ver, vnull)
    return be.L.rl_debug_verdict(be.ctx, nq, n, *[None if k in null else abi.ptr(x) for k, x in cols.items()], opts,
                                 None if no_verdict else C.byref(v))


def _debug_respond(be, nq=NQ, n=N, req=(0, 0, 1, 1), status=None, no_resp=False, rnull=(), no_ans=False, anull=(), opts=0,
                   keys=KEYS, fmt=None, bytes_cap=None, reset=0, null_req=False):
    a = _answers(n)
    a["reset_s"][:] = reset
    req = np.array(list(req) + [0] * max(n - len(req), 0), np.uint32)
    r = _struct(abi.RlRequestResult, a, anull)
    f, keep = abi.make_response_format(keys)
    for k, x in (fmt or {}).items():
        setattr(f, k, x)
    rb = _struct(abi.RlResponseBatch, be.resp, rnull)
    rb.bytes_cap = len(be.resp["bytes"]) if bytes_cap is None else bytes_cap
    st = None if status is None else np.array(status, np.uint8)
    return be.L.rl_debug_respond(be.ctx, nq, n, None if null_req else abi.ptr(req), abi.ptr(st),
                                 None if no_ans else C.byref(r), opts, C.byref(f), None if no_resp else C.byref(rb))


DEBUG_VERDICT = [("null_verdict", lambda be: _debug_verdict(be, no_verdict=True)),
                 ("verdict_without_overall_code", lambda be: _debug_verdict(be, vnull=("overall_code",))),
                 ("unknown_option", lambda be: _debug_verdict(be, opts=2)),
                 ("descriptors_over_max_batch", lambda be: _debug_verdict(be, n=MAX_BATCH + 1)),
                 ("requests_over_max_requests", lambda be: _debug_verdict(be, nq=MAX_REQUESTS + 1))] + \
    [("null_" + k, lambda be, k=k: _debug_verdict(be, null=(k,)))
     for k in ("req_idx", "match", "code", "limit_remaining", "reset_s", "requests_per_unit")] + \
    [("req_idx_decreasing", lambda be: _debug_verdict(be, req=(0, 1, 0, 1))),
     ("req_idx_at_n_requests", lambda be: _debug_verdict(be, req=(0, 0, 1, NQ)))]
DEBUG_RESPOND = [("null_resp", lambda be: _debug_respond(be, no_resp=True)),
                 ("null_resp_off", lambda be: _debug_respond(be, rnull=("resp_off",))),
                 ("null_answers", lambda be: _debug_respond(be, no_ans=True)),
                 ("unknown_option", lambda be: _debug_respond(be, opts=2)),
                 ("format_key_over_64", lambda be: _debug_respond(be, keys=(b"k" * 65, b"r", b"s"))),
                 ("format_null_key_with_length", lambda be: _debug_respond(be, keys=None, fmt={"limit_key_len": 3})),
                 ("format_reserved", lambda be: _debug_respond(be, fmt={"reserved": 1})),
                 ("descriptors_over_max_batch", lambda be: _debug_respond(be, n=MAX_BATCH + 1)),
                 ("requests_over_max_requests", lambda be: _debug_respond(be, nq=MAX_REQUESTS + 1)),
                 ("null_req_idx", lambda be: _debug_respond(be, null_req=True))] + \
    [("null_answer_" + k, lambda be, k=k: _debug_respond(be, anull=(k,)))
     for k in ("match", "code", "limit_remaining", "reset_s", "requests_per_unit", "unit")] + \
    [("req_idx_decreasing", lambda be: _debug_respond(be, req=(0, 1, 0, 1))),
     ("req_idx_at_n_requests", lambda be: _debug_respond(be, req=(0, 0, 1, NQ))),
     ("deferred_request_with_descriptors", lambda be: _debug_respond(be, status=(0, abi.RL_WIRE_DEFERRED))),
     ("reset_s_at_2_21", lambda be: _debug_respond(be, reset=1 << 21)),
     ("resp_without_bytes", lambda be: _debug_respond(be, rnull=("bytes",))),
     ("bound_over_bytes_cap", lambda be: _debug_respond(be, bytes_cap=8))]


# ---- the override-rules calls -------------------------------------------------------------------

def _ov_enable(be, none=False, first=4, capacity=4, reserved=0):
    cfg = abi.RlOverrideRulesConfig()
    cfg.first_rule, cfg.capacity, cfg.reserved[1] = first, capacity, reserved
    return be.L.rl_override_rules_enable(be.ctx, None if none else C.byref(cfg))


def _ov_info(be, none=False):
    info = abi.RlOverrideRulesInfo()
    return be.L.rl_override_rules_info_get(be.ctx, None if none else C.byref(info))


def _ov_keys(be, first=4, n=0, no_off=False):
    off, need = np.zeros(n + 2, np.uint32), C.c_uint64(0)
    return be.L.rl_override_rule_keys(be.ctx, first, n, None, 0, None if no_off else abi.ptr(off), C.byref(need))


def _ov_valid_enable(be):
    """rl_override_rules_enable succeeds once per ctx: after that, a second try is the 'already enabled' refusal."""
    if be.ov_enabled:
        return abi.RL_OK if _ov_enable(be) == abi.RL_E_INVALID else abi.RL_E_INTERNAL
    be.ov_enabled = True
    return _ov_enable(be)


# (rl_override_rules_enable looks at `already enabled` first: its other refusals come before the ctx enables)
OV_BEFORE = [("info_get_not_enabled", _ov_info), ("rule_keys_not_enabled", _ov_keys),
             ("enable_null_config", lambda be: _ov_enable(be, none=True)),
             ("enable_reserved", lambda be: _ov_enable(be, reserved=1)),
             ("enable_capacity_zero", lambda be: _ov_enable(be, capacity=0)),
             ("enable_beyond_max_rules", lambda be: _ov_enable(be, first=MAX_RULES - 1, capacity=2))]
OV_ENABLE = [("already_enabled", _ov_enable)]
OV_INFO = [("null_info", lambda be: _ov_info(be, none=True))]
OV_KEYS = [("null_off", lambda be: _ov_keys(be, no_off=True)),
           ("range_below_first_rule", lambda be: _ov_keys(be, first=3)),
           ("range_beyond_handed_out", lambda be: _ov_keys(be, n=1))]


def _single(call):
    """A family of the single-shard calls on a ctx of two shards: its one refusal, and no valid call."""
    return [("single_shard_only", call)]


def families(shards, pr):
    """-> [(entry point, its valid call or None, [(case, the refused call)])]: issued in this order, which is part
    of the fixture; pr: the ctx, for its batches' sizes. (A one-shard ctx's rl_last_error keeps the engine's previous
    text after a refusal that rl_api.hip makes through plain `fail`: DESIGN.md section 11, open item.)"""
    fam = [("requests", lambda be: _requests_call(be, verdict=False), REQUESTS_PLAIN),
           ("requests_verdict", _requests_call, REQUESTS),
           ("compact", lambda be: _hostfed_call(be, "compact"), _compact_cases(pr)),
           ("prefixed", lambda be: _hostfed_call(be, "prefixed"), _prefixed_cases(pr)),
           ("debug_verdict", _debug_verdict, DEBUG_VERDICT),
           ("debug_respond", _debug_respond, DEBUG_RESPOND)]
    if shards == 1:
        fam += [("packed", _packed_call, _packed_cases(pr)),
                ("wire", _wire_call, _wire_cases(pr, False)),
                ("wire_respond", lambda be: _wire_call(be, True), _wire_cases(pr, True)),
                ("override_rules_before_enable", None, OV_BEFORE),
                ("override_rules_enable", _ov_valid_enable, OV_ENABLE),
                ("override_rules_info_get", _ov_info, OV_INFO),
                ("override_rule_keys", _ov_keys, OV_KEYS),
                # (with override rules on, the wire path carves one piece more: its two late refusals again)
                ("wire_with_override_rules", _wire_call, _wire_cases(pr, False)[-2:])]
    else:
        fam += [("packed", None, _single(_packed_call)), ("wire", None, _single(_wire_call)),
                ("wire_respond", None, _single(lambda be: _wire_call(be, True))),
                ("override_rules_enable", None, _single(_ov_enable)),
                ("override_rules_info_get", None, _single(_ov_info)),
                ("override_rule_keys", None, _single(_ov_keys))]
    return fam


NO_CONFIG = [("requests", lambda be: _requests_call(be, verdict=False)), ("requests_verdict", _requests_call),
             ("packed", _packed_call), ("wire", _wire_call), ("wire_respond", lambda be: _wire_call(be, True))]


def run_cases(shards):
    """-> [[case id, return code, rl_last_error text]] of every refused call, in order."""
    got = []

    def refused(be, cid, call, valid):
        before = be.table_info()
        rc = call(be)
        msg = be.L.rl_last_error(be.ctx).decode()
        print("%d shard(s) %s -> %d %r" % (shards, cid, rc, msg))
        got.append([cid, rc, msg])
        assert rc != abi.RL_OK, "%s was not refused" % cid
        assert be.L.rl_synchronize(be.ctx) == abi.RL_OK, "%s: reported twice" % cid
        assert be.table_info() == before, "%s changed the table" % cid
        if valid is not None:
            assert valid(be) == abi.RL_OK, "a valid call after %s: %s" % (cid, be.L.rl_last_error(be.ctx))

    be = Ctx(shards)
    try:
        for name, valid, cases in families(shards, be):
            if valid is not None:
                assert valid(be) == abi.RL_OK, "%s: %s" % (name, be.L.rl_last_error(be.ctx))
            for case, call in cases:
                refused(be, "%s.%s" % (name, case), call, valid)
    finally:
        be.close()
    bare = Ctx(shards, config=False)
    try:
        for name, call in NO_CONFIG[:2 if shards > 1 else None]:
            refused(bare, "%s.no_config" % name, call, None)
    finally:
        bare.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [1, 2])
def test_request_argument_errors_are_as_recorded(shards):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"][str(shards)]
    got = run_cases(shards)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_request_errors.py --record")
    rec = {str(s): run_cases(s) for s in (1, 2)}
    doc = {"kind": "own", "comment": "Return codes and rl_last_error texts of the request path's host-side refusals, "
           "recorded from the library before its host side was gathered into rl_requests.hip "
           "(tests/test_gpu_request_errors.py --record). Never re-recorded from the code under test.",
           "cases": rec}
    out = os.environ.get("RL_RECORD_TO", GOLDEN)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("recorded %d + %d cases" % (len(rec["1"]), len(rec["2"])))
