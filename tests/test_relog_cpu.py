"""CPU-side checks of rl_resize_history and rl_resize_arena: the header declares
them and the library exports them under ABI 8 (symbols and types only added);
the ctypes mirror of rl_history_resize_info equals the C compiler's layout of
include/ratelimit_hip.h field for field (tests/c_abi/relog_layout.c); the
rounding rule rl_log_geom.h, compiled for the host plain and under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program, gives
the sizes rl_create has always given (tests/c_abi/log_geom_run.cpp);
Backend.resize_history / resize_arena pass their arguments through, return the
info's fields, follow the new sizes in their config and raise with the status
(a stub library: no device)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from ratelimit_amd import abi, _lib
from ratelimit_amd.limiter import Backend, RedisError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "ratelimit_hip.h")
CSRC = os.path.join(ROOT, "ratelimit_amd", "csrc")
LIB = os.path.join(ROOT, "ratelimit_amd", "libratelimit_hip.so")
CFLAGS = ["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]

# (history_entries, max_batch) -> entries per partition, worked out by hand from
# the rule "a power of two, at least max(history_entries / 64, max_batch / 16,
# 1024), at most 2^25": the 1024 floor, the batch floor, the request's own
# floor, the cap, exact powers of two and one partition's worth above.
# tests/test_gpu_resize.py and test_gpu_history.py pin the first rows on a ctx.
PINNED = [
    (1, 1 << 14, 1024), (1 << 16, 1 << 14, 1024), ((1 << 16) + 64, 1 << 14, 2048), (1 << 18, 1 << 14, 4096),
    (1 << 20, 1 << 20, 65536), (1, 1 << 20, 65536), (1, 8388608, 524288), (1 << 31, 1 << 14, 1 << 25),
    ((1 << 31) - 1, 1, 1 << 25), ((1 << 30) + 64, 1 << 16, 1 << 25), (1 << 27, 1 << 20, 1 << 21),
    ((1 << 27) + 63, 1 << 20, 1 << 21), ((1 << 27) + 64, 1 << 20, 1 << 22), (65535, 1, 1024), (65536 + 63, 1, 1024),
    (1 << 28, 1 << 22, 1 << 22),
]


def test_header_declares_and_library_exports_the_calls():
    src = open(HEADER).read()
    assert ("int rl_resize_history(rl_ctx* ctx, uint64_t history_entries, "
            "rl_history_resize_info* info /* may be NULL */);") in src
    assert "int rl_resize_arena(rl_ctx* ctx, uint64_t arena_bytes);" in src
    assert "#define RL_ABI_VERSION 8u" in src
    assert "rl_resize_history" in _lib.EXPORTS and "rl_resize_arena" in _lib.EXPORTS
    if not os.path.exists(LIB):
        from ratelimit_amd import build
        build.build()
    lib = C.CDLL(LIB)
    assert hasattr(lib, "rl_resize_history") and hasattr(lib, "rl_resize_arena")
    lib.rl_abi_version.restype = C.c_uint32
    assert lib.rl_abi_version() == abi.ABI_VERSION == 8


def test_history_resize_info_matches_the_c_layout(tmp_path):
    exe = str(tmp_path / "relog_layout")
    subprocess.run(CFLAGS + [os.path.join(ROOT, "tests", "c_abi", "relog_layout.c"), "-o", exe], check=True,
                   capture_output=True, text=True)
    sizes, fields, consts = {}, [], {}
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] == "S":
            sizes[p[1]] = int(p[2])
        elif p[0] == "F":
            fields.append((p[2], int(p[3]), int(p[4])))
        else:
            consts[p[1]] = int(p[2])
    cls = abi.RlHistoryResizeInfo
    assert sizes == {"rl_history_resize_info": C.sizeof(cls)} and C.sizeof(cls) == 72
    assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == fields
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION}


def test_the_library_sizes_the_log_by_the_shared_header():
    """eng_create (rl_engine.hip) and rl_resize_history (rl_maint.hip) both call rl_log_geom.h; nothing restates
    the rule."""
    eng = open(os.path.join(CSRC, "rl_engine.hip")).read()
    maint = open(os.path.join(CSRC, "rl_maint.hip")).read()
    assert '#include "rl_log_geom.h"' in eng and '#include "rl_log_geom.h"' in maint
    assert eng.count("log_part_cap(") == 1 and maint.count("log_part_cap(") == 1
    assert "cap * 2 <= want" not in eng + maint
    from ratelimit_amd import build
    assert "rl_relog.hip" in build.SOURCES and "rl_log_geom.h" in build.HEADERS and "rl_chain.h" in build.HEADERS
    assert "rl_maint.hip" in build.SOURCES and "rl_engine_int.h" in build.HEADERS


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_log_geometry_on_the_host(tmp_path, flags):
    """log_part_cap against the rule as rl_create states it (restated in the
    program) on every pinned request, every power of two with its neighbours
    under four batch sizes and 20 000 random requests; the pinned requests'
    sizes against the hand-worked table above."""
    assert shutil.which("g++"), "the host build of rl_log_geom.h needs g++"
    exe = str(tmp_path / "log_geom_run")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "log_geom_run.cpp"), "-o", exe] + flags, check=True,
                   capture_output=True, text=True)
    if flags is SAN:
        syms = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
        assert "__asan_" in syms and "__ubsan_handle" in syms  # (instrumented)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.split("\n")
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("cap ")]
    assert got == PINNED
    ok = [ln for ln in lines if ln.startswith("ok ")]
    assert ok and int(ok[0].split()[1]) >= 20000


# --------------------------------------------------------------------------- the wrappers over a stub library
class _StubLib:
    def __init__(self, rc=abi.RL_OK):
        self.rc, self.calls = rc, []

    def rl_resize_history(self, ctx, entries, iref):
        self.calls.append(("history", ctx, entries))
        if self.rc != abi.RL_OK:
            return self.rc
        info = iref._obj
        info.entries_before, info.entries_after = 2 << 16, 2 << 18  # (two shards)
        info.written_before, info.entries_kept, info.entries_dropped = 5000, 3000, 2000
        info.chains, info.chains_lost, info.fill_max, info.longest_chain, info.reserved = 900, 7, 61, 9, 0
        return abi.RL_OK

    def rl_resize_arena(self, ctx, nbytes):
        self.calls.append(("arena", ctx, nbytes))
        return self.rc

    def rl_last_error(self, ctx):
        return b"gpu: rl_resize_history: stub"

    def rl_destroy(self, ctx):
        pass


def _stub_backend(rc=abi.RL_OK, n_shards=2):
    be = Backend.__new__(Backend)  # (no rl_create: no device)
    be.L, be.ctx, be.cfg = _StubLib(rc), 1234, abi.RlConfig()
    be.cfg.n_shards, be.cfg.history_entries, be.cfg.arena_bytes = n_shards, 1 << 16, 1 << 20
    return be


def test_backend_resize_history_passes_through_and_returns_the_info():
    be = _stub_backend()
    got = be.resize_history(200_000)
    assert be.L.calls == [("history", 1234, 200_000)]
    assert got == {"entries_before": 2 << 16, "entries_after": 2 << 18, "written_before": 5000, "entries_kept": 3000,
                   "entries_dropped": 2000, "chains": 900, "chains_lost": 7, "fill_max": 61, "longest_chain": 9}
    assert be.cfg.history_entries == 1 << 18  # (per shard, rounded: what a fresh ctx for its snapshot needs)


def test_backend_resize_arena_passes_through():
    be = _stub_backend()
    assert be.resize_arena(1 << 22) is None
    assert be.L.calls == [("arena", 1234, 1 << 22)] and be.cfg.arena_bytes == 1 << 22


@pytest.mark.parametrize("rc,name", [(abi.RL_E_INVALID, "RL_E_INVALID"), (abi.RL_E_CAPACITY, "RL_E_CAPACITY"),
                                     (abi.RL_E_ARENA_FULL, "RL_E_ARENA_FULL"), (abi.RL_E_HIP, "RL_E_HIP")])
def test_backend_failures_raise_with_the_status_and_keep_the_config(rc, name):
    be = _stub_backend(rc=rc)
    with pytest.raises(RedisError, match=name) as ei:
        be.resize_history(1 << 20)
    assert ei.value.status == rc and "stub" in str(ei.value)
    with pytest.raises(RedisError, match=name):
        be.resize_arena(1 << 24)
    assert be.cfg.history_entries == 1 << 16 and be.cfg.arena_bytes == 1 << 20 and len(be.L.calls) == 2
