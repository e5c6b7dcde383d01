"""CPU-side checks of rl_hot_keys: the header declares it and the library
exports it under ABI 8; the ctypes mirrors of rl_hot_query / rl_hot_info equal
the C compiler's layout of include/ratelimit_hip.h field for field;
Backend.hot_keys builds the query, sizes its buffers from k and retries once on
RL_E_CAPACITY (a stub library: no device); rl_hot_select.h, compiled for the
host, selects, orders and merges like a plain sort (tests/c_abi/hot_select_run.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from ratelimit_amd import abi, _lib
from ratelimit_amd.limiter import Backend, FixedTimeSource, GpuRateLimitCache, HotKey, RedisError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "ratelimit_hip.h")
LIB = os.path.join(ROOT, "ratelimit_amd", "libratelimit_hip.so")
CFLAGS = ["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC]

MIRROR = {"rl_hot_query": abi.RlHotQuery, "rl_hot_info": abi.RlHotInfo}


def test_header_declares_and_library_exports_rl_hot_keys():
    src = open(HEADER).read()
    assert "int rl_hot_keys(rl_ctx* ctx, const rl_hot_query* q, rl_records* out, rl_hot_info* info);" in src
    assert "#define RL_ABI_VERSION 8u" in src
    assert "#define RL_HOT_BLOCKED 0x1u" in src
    assert "rl_hot_keys" in _lib.EXPORTS
    if not os.path.exists(LIB):
        from ratelimit_amd import build
        build.build()
    lib = C.CDLL(LIB)
    assert hasattr(lib, "rl_hot_keys")
    lib.rl_abi_version.restype = C.c_uint32
    assert lib.rl_abi_version() == abi.ABI_VERSION == 8


def test_hot_structs_match_the_c_layout(tmp_path):
    exe = str(tmp_path / "hot_layout")
    subprocess.run(CFLAGS + [os.path.join(ROOT, "tests", "c_abi", "hot_layout.c"), "-o", exe], check=True,
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
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION, "RL_HOT_BLOCKED": abi.RL_HOT_BLOCKED}
    assert C.sizeof(abi.RlHotQuery) == 24 and C.sizeof(abi.RlHotInfo) == 48


def test_hot_select_header_on_the_host(tmp_path):
    """The predicate, the order and the 2- / 3-way merge of rl_hot_select.h
    against a plain sort (counts on the radix digit boundaries, empty sets,
    k larger than the set, every record tied)."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "hot_select_run")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra",
                    "-I" + os.path.join(ROOT, "ratelimit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_abi", "hot_select_run.cpp"), "-o", exe], check=True,
                   capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) >= 400


class StubLib:
    """Stands for the library: records what rl_hot_keys was given. The table it
    plays holds `table` = [(stem, unit, count)], every record matching; an
    `out` too small for min(k, len(table)) records or their stems is
    RL_E_CAPACITY with info filled and out untouched."""

    def __init__(self, table, fail_always=False):
        self.table = sorted(table, key=lambda r: (-r[2], r[0], r[1]))
        self.calls = []
        self.fail_always = fail_always

    def rl_hot_keys(self, ctx, qref, rref, iref):
        q, r, info = qref._obj, rref._obj, iref._obj
        self.calls.append({"now": q.now, "k": q.k, "min_count": q.min_count, "unit_mask": q.unit_mask,
                           "flags": q.flags, "n": r.n, "stem_cap": r.stem_cap})
        top = self.table[:q.k]
        info.slots, info.matched = 1024, len(self.table)
        info.hits = sum(t[2] for t in self.table)
        info.threshold = top[-1][2] if top else 0
        info.above = sum(t[2] > info.threshold for t in top)
        info.time_floor = 5
        nb = sum(len(t[0]) for t in top)
        if self.fail_always or len(top) > r.n or nb > r.stem_cap:
            return abi.RL_E_CAPACITY

        def arr(p, dt, m):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), (max(m, 1),))

        n = len(top)
        off = arr(r.stem_off, C.c_uint32, n + 1)
        blob = arr(r.stem_bytes, C.c_uint8, nb)
        off[0] = 0
        for i, (stem, unit, count) in enumerate(top):
            blob[off[i]:off[i] + len(stem)] = np.frombuffer(stem, np.uint8)
            off[i + 1] = off[i] + len(stem)
            arr(r.unit, C.c_uint8, n)[i] = unit
            arr(r.flags, C.c_uint8, n)[i] = 0
            arr(r.ws, C.c_uint32, n)[i] = q.now - q.now % 60
            arr(r.count, C.c_uint32, n)[i] = count
            arr(r.expire, C.c_uint32, n)[i] = q.now + 60
            arr(r.lc, C.c_uint32, n)[i] = q.now + 7 if unit == 3 else 0
        r.n = n
        return abi.RL_OK

    def rl_last_error(self, ctx):
        return b"gpu: rl_hot_keys: larger than rl_records (stub)"


def _stub_backend(table, **kw):
    be = Backend.__new__(Backend)
    be.L = StubLib(table, **kw)
    be.ctx = None  # (close() then has nothing to destroy)
    be.cfg = abi.RlConfig()
    be.cfg.max_batch, be.cfg.n_shards = 1 << 12, 1
    return be


def _stems(rec):
    off, sb = rec["stem_off"], rec["stem_bytes"]
    return [bytes(sb[off[i]:off[i + 1]]) for i in range(len(rec["ws"]))]


SHORT = [(b"stem_%03d_" % j, 1 + j % 4, 1 + (j * 37) % 101) for j in range(300)]


def test_hot_keys_builds_the_query_and_sizes_the_buffers_from_k():
    be = _stub_backend(SHORT)
    rec, info = be.hot_keys(1_700_000_123, 10)
    (call,) = be.L.calls
    assert call["now"] == 1_700_000_123 and call["k"] == 10 and call["min_count"] == 0
    assert call["unit_mask"] == 0 and call["flags"] == 0
    assert call["n"] == 10 and call["stem_cap"] >= 128 * 10
    want = be.L.table[:10]
    assert _stems(rec) == [t[0] for t in want] and list(rec["count"]) == [t[2] for t in want]
    assert list(rec["unit"]) == [t[1] for t in want] and not rec["flags"].any()
    assert set(rec) == {"stem_bytes", "stem_off"} | set(abi.RECORD_DTYPES)
    for f, dt in abi.RECORD_DTYPES.items():
        assert rec[f].dtype == dt and len(rec[f]) == 10, f
    assert info == {"slots": 1024, "matched": 300, "hits": sum(t[2] for t in SHORT), "above": info["above"],
                    "threshold": want[-1][2], "time_floor": 5}
    # the unit mask: bit u per selected unit; the flag
    for units, mask in (([1], 2), ([2], 4), ([3, 4], 24), ((1, 2, 3, 4), 30), ([], 0), (None, 0)):
        be.hot_keys(77, 3, min_count=5, units=units, blocked=True)
        call = be.L.calls[-1]
        assert (call["unit_mask"], call["flags"], call["min_count"], call["now"]) == (mask, abi.RL_HOT_BLOCKED, 5, 77)
    # k = 0: only info; k past the table: everything
    rec, info = be.hot_keys(77, 0)
    assert len(rec["ws"]) == 0 and len(rec["stem_bytes"]) == 0 and info["matched"] == 300
    n_calls = len(be.L.calls)
    rec, _ = be.hot_keys(77, 4096)
    assert len(rec["ws"]) == 300 and be.L.calls[-1]["n"] == 4096 and len(be.L.calls) == n_calls + 1


def test_hot_keys_retries_once_with_buffers_sized_from_info():
    long_table = [(bytes([65 + j % 26]) * (3000 + j), 2, 1000 - j) for j in range(40)] + SHORT
    be = _stub_backend(long_table)
    rec, info = be.hot_keys(500, 64)  # 40 stems of 3 KB: over the first attempt's 64 KiB
    first, second = be.L.calls
    assert first["n"] == 64 and first["stem_cap"] == 1 << 16
    assert second["n"] == min(64, info["matched"]) == 64 and second["stem_cap"] == 64 * 65535
    assert _stems(rec) == [t[0] for t in be.L.table[:64]]
    longer = [(bytes([65 + j % 26]) * (20000 + j), 2, 1000 - j) for j in range(40)] + SHORT[:5]
    be = _stub_backend(longer)
    rec, info = be.hot_keys(500, 4000)  # fewer records than k: the retry asks for what matched
    assert [(c["n"], c["stem_cap"]) for c in be.L.calls] == [(4000, 128 * 4000), (45, 45 * 65535)]
    assert len(rec["ws"]) == 45 and _stems(rec) == [t[0] for t in be.L.table]
    be = _stub_backend(SHORT, fail_always=True)
    with pytest.raises(RedisError, match="RL_E_CAPACITY") as e:
        be.hot_keys(500, 10)
    assert e.value.status == abi.RL_E_CAPACITY and len(be.L.calls) == 2  # one retry, then the failure


def test_cache_hot_keys_reads_the_time_source():
    cache = GpuRateLimitCache.__new__(GpuRateLimitCache)
    cache.time_source = FixedTimeSource(1_700_000_123)
    cache.prefix = ""
    cache.backend = _stub_backend(SHORT)
    got = cache.hot_keys(5)
    assert cache.backend.L.calls[-1]["now"] == 1_700_000_123
    want = cache.backend.L.table[:5]
    assert got == [HotKey(s, u, 1_700_000_123 - 1_700_000_123 % 60, c, 1_700_000_183,
                          1_700_000_130 if u == 3 else 0) for s, u, c in want]
    assert got[0].count >= got[-1].count
    cache.hot_keys(5, now=99, min_count=3, units=[2], blocked=True)
    call = cache.backend.L.calls[-1]
    assert (call["now"], call["min_count"], call["unit_mask"], call["flags"]) == (99, 3, 4, 1)
