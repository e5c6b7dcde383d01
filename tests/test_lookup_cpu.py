"""CPU-side checks of the keyed lookup (rl_lookup): the header declares it and
the library exports it under ABI 8; the ctypes mirrors of rl_keys /
rl_key_state equal the C compiler's layout of include/ratelimit_hip.h field for
field; Backend.lookup splits its keys into calls the ctx accepts and
GpuRateLimitCache.peek builds do_limit's stems (a stub library: no device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from ratelimit_amd import abi, _lib
from ratelimit_amd.limiter import Backend, FixedTimeSource, GpuRateLimitCache, KeyState, RedisError
from ratelimit_amd.packing import pack_calls, RuleInterner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "ratelimit_hip.h")
LIB = os.path.join(ROOT, "ratelimit_amd", "libratelimit_hip.so")
CFLAGS = ["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC]

MIRROR = {"rl_keys": abi.RlKeys, "rl_key_state": abi.RlKeyState}


def test_header_declares_and_library_exports_rl_lookup():
    src = open(HEADER).read()
    assert "int rl_lookup(rl_ctx* ctx, const rl_keys* in, rl_key_state* out);" in src
    assert "#define RL_ABI_VERSION 8u" in src
    assert "rl_lookup" in _lib.EXPORTS
    if not os.path.exists(LIB):
        from ratelimit_amd import build
        build.build()
    lib = C.CDLL(LIB)
    assert hasattr(lib, "rl_lookup")
    lib.rl_abi_version.restype = C.c_uint32
    assert lib.rl_abi_version() == abi.ABI_VERSION == 8


def test_lookup_structs_match_the_c_layout(tmp_path):
    exe = str(tmp_path / "lookup_layout")
    subprocess.run(CFLAGS + [os.path.join(ROOT, "tests", "c_abi", "lookup_layout.c"), "-o", exe], check=True,
                   capture_output=True, text=True)
    sizes, fields, consts = {}, {}, {}
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] == "S":
            sizes[p[1]] = int(p[2])
        elif p[0] == "F":
            fields.setdefault(p[1], []).append((p[2], int(p[3]), int(p[4])))
        else:
            consts[p[1]] = int(p[2])
    assert set(sizes) == set(MIRROR)
    for name, cls in MIRROR.items():
        assert C.sizeof(cls) == sizes[name], name
        mirror = [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]
        assert mirror == fields[name], name  # the same fields in the same order, offsets and sizes
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION}
    assert C.sizeof(abi.RlKeys) == 8 + 4 * 8 and C.sizeof(abi.RlKeyState) == 5 * 8
    assert set(abi.KEY_STATE_DTYPES) == {f for f, _ in abi.RlKeyState._fields_}


class StubLib:
    """Stands for the library: records what rl_lookup was given and answers
    count = the stem's length, expire = now + unit, found = 1, lc = 0; a stem
    starting with "T" gets status RL_E_TIME."""

    def __init__(self, fail_at=None):
        self.calls = []
        self.fail_at = fail_at

    def rl_lookup(self, ctx, kref, sref):
        k, s = kref._obj, sref._obj
        n = k.n

        def arr(p, dt, m):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), (m,))

        off = arr(k.stem_off, C.c_uint32, n + 1).copy()
        stem = arr(k.stem_bytes, C.c_uint8, max(int(off[n]), 1)).copy()[:int(off[n])]
        unit, now = arr(k.unit, C.c_uint8, n).copy(), arr(k.now, C.c_int64, n).copy()
        self.calls.append({"stem_off": off, "stem_bytes": stem, "unit": unit, "now": now})
        if self.fail_at == len(self.calls):
            return abi.RL_E_CAPACITY
        lens = np.diff(off.astype(np.int64))
        bad = np.array([stem[off[i]] == ord("T") if lens[i] else False for i in range(n)], bool)
        arr(s.status, C.c_uint8, n)[:] = np.where(bad, abi.RL_E_TIME, 0)
        arr(s.found, C.c_uint8, n)[:] = ~bad
        arr(s.count, C.c_uint32, n)[:] = np.where(bad, 0, lens)
        arr(s.expire, C.c_uint32, n)[:] = np.where(bad, 0, now + unit)
        arr(s.lc, C.c_uint32, n)[:] = np.where(unit == 3, now + 7, 0)
        return abi.RL_OK

    def rl_last_error(self, ctx):
        return b"gpu: lookup exceeds configured max_batch (stub)"


def _stub_backend(max_batch, max_stem_bytes=0, **kw):
    be = Backend.__new__(Backend)
    be.L = StubLib(**kw)
    be.ctx = None  # (close() then has nothing to destroy)
    be.cfg = abi.RlConfig()
    be.cfg.max_batch, be.cfg.max_stem_bytes, be.cfg.n_shards = max_batch, max_stem_bytes, 1
    return be


def _keys(n, seed=0):
    rng = np.random.default_rng(seed)
    stems = [bytes(rng.integers(97, 123, int(L)).astype(np.uint8)) for L in rng.integers(1, 70, n)]
    return stems, rng.integers(1, 5, n).astype(np.uint8), rng.integers(10**9, 2 * 10**9, n).astype(np.int64)


def _check_joined(be, stems, units, nows, res):
    calls = be.L.calls
    got = []
    for c in calls:  # every call is a batch of its own: offsets rebased, stems cut to match
        assert c["stem_off"][0] == 0 and len(c["stem_bytes"]) == c["stem_off"][-1]
        got += [bytes(c["stem_bytes"][c["stem_off"][i]:c["stem_off"][i + 1]]) for i in range(len(c["unit"]))]
    assert got == list(stems)
    assert np.array_equal(np.concatenate([c["unit"] for c in calls]), units)
    assert np.array_equal(np.concatenate([c["now"] for c in calls]), nows)
    assert set(res) == set(abi.KEY_STATE_DTYPES)
    for k, dt in abi.KEY_STATE_DTYPES.items():
        assert res[k].dtype == dt and len(res[k]) == len(stems), k
    assert np.array_equal(res["count"], [len(s) for s in stems])  # each call's answers land at its keys
    assert np.array_equal(res["expire"], nows + units) and res["found"].all() and not res["status"].any()
    assert np.array_equal(res["lc"], np.where(units == 3, nows + 7, 0))


def test_lookup_splits_at_max_batch():
    stems, units, nows = _keys(2500)
    be = _stub_backend(1000)
    res = be.lookup(stems, units, nows)
    assert [len(c["unit"]) for c in be.L.calls] == [1000, 1000, 500]
    _check_joined(be, stems, units, nows, res)
    be = _stub_backend(500)  # an exact multiple
    be.lookup(*_keys(1000, 1))
    assert [len(c["unit"]) for c in be.L.calls] == [500, 500]
    be = _stub_backend(0)  # (0: the library's default, 1 << 20)
    _check_joined(be, stems, units, nows, be.lookup(stems, units, nows))
    assert len(be.L.calls) == 1
    be = _stub_backend(10)  # no keys: no call, empty arrays
    res = be.lookup([], [], [])
    assert be.L.calls == [] and all(len(v) == 0 for v in res.values())


def test_lookup_splits_at_max_stem_bytes():
    stems, units, nows = _keys(400, 2)
    be = _stub_backend(1000, max_stem_bytes=1024)
    res = be.lookup(stems, units, nows)
    assert len(be.L.calls) > 1 and all(c["stem_off"][-1] <= 1024 for c in be.L.calls)
    _check_joined(be, stems, units, nows, res)


def test_lookup_passes_key_statuses_and_raises_call_failures():
    be = _stub_backend(100)
    res = be.lookup([b"abc", b"Tardy", b"", b"zz"], [1, 2, 1, 3], [50, 60, 70, 80])
    assert list(res["status"]) == [0, abi.RL_E_TIME, 0, 0] and list(res["found"]) == [1, 0, 1, 1]
    assert list(res["count"]) == [3, 0, 0, 2] and list(res["lc"]) == [0, 0, 0, 87]
    with pytest.raises(ValueError):
        be.lookup([b"a", b"b"], [1], [5, 5])
    be = _stub_backend(100, fail_at=2)
    with pytest.raises(RedisError, match="RL_E_CAPACITY") as e:
        be.lookup(*_keys(250, 3))
    assert e.value.status == abi.RL_E_CAPACITY and len(be.L.calls) == 2  # stops at the failed call


def _stub_cache(prefix="", now=1_700_000_123, **kw):
    cache = GpuRateLimitCache.__new__(GpuRateLimitCache)
    cache.time_source = FixedTimeSource(now)
    cache.prefix = prefix
    cache.backend = _stub_backend(1 << 10, **kw)
    return cache


def test_peek_builds_do_limits_stems():
    sec = O.new_rate_limit(10, O.SECOND, "k_sec")
    hour = O.new_rate_limit(10, O.HOUR, "k_hour")
    req = O.RateLimitRequest("dom", [O.Descriptor([("a", "1")]), O.Descriptor([("nil", "x")]),
                                     O.Descriptor([("b", "2"), ("c", "3")])], 4)
    limits = [sec, None, hour]
    for prefix in ("", "pfx:"):
        cache = _stub_cache(prefix)
        got = cache.peek(req, limits)
        pb = pack_calls([(req, limits, 1_700_000_123)], prefix, RuleInterner())  # what do_limit sends
        (call,) = cache.backend.L.calls
        assert np.array_equal(call["stem_bytes"], pb.arrays["stem_bytes"][:pb.arrays["stem_off"][-1]])
        assert np.array_equal(call["stem_off"], pb.arrays["stem_off"])
        assert np.array_equal(call["unit"], pb.arrays["unit"]) and list(call["now"]) == [1_700_000_123] * 2
        la, lb = len(prefix) + len("dom_a_1_"), len(prefix) + len("dom_b_2_c_3_")
        assert got == [KeyState(la, 1, False), None, KeyState(lb, 3, True)]
        assert got[0].ttl_s == 1 and got[2].over_limit_cached
    cache = _stub_cache()
    assert cache.peek(req, limits, now=77)[0] == KeyState(8, 1, False)  # an explicit clock
    assert list(cache.backend.L.calls[0]["now"]) == [77, 77]
    assert cache.peek(O.RateLimitRequest("dom", [O.Descriptor([("a", "1")])], 1), [None]) == [None]
    assert len(cache.backend.L.calls) == 1  # nil limits only: no call
    with pytest.raises(AssertionError):
        cache.peek(req, [sec])


def test_peek_raises_on_a_failed_key_and_reports_missing_keys():
    cache = _stub_cache()
    lim = O.new_rate_limit(10, O.MINUTE, "k")
    with pytest.raises(RedisError, match="RL_E_TIME") as e:
        cache.peek(O.RateLimitRequest("Tdom", [O.Descriptor([("a", "1")])], 1), [lim])
    assert e.value.status == abi.RL_E_TIME

    def not_found(ctx, kref, sref):  # a key that does not exist: found 0, everything 0
        return abi.RL_OK

    cache.backend.L.rl_lookup = not_found
    assert cache.peek(O.RateLimitRequest("dom", [O.Descriptor([("a", "1")])], 1), [lim]) == [KeyState(0, None, False)]
