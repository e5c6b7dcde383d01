"""CPU-side checks of rl_resize: the header declares it and the library exports
it under ABI 8 (symbols and types only added); the ctypes mirror of
rl_resize_info equals the C compiler's layout of include/ratelimit_hip.h field
for field (tests/c_abi/resize_layout.c); Backend.resize passes the size through
and returns the info's fields (a stub library: no device)."""
import ctypes as C
import os
import subprocess

import pytest

from ratelimit_amd import abi, _lib
from ratelimit_amd.limiter import Backend, RedisError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "ratelimit_hip.h")
LIB = os.path.join(ROOT, "ratelimit_amd", "libratelimit_hip.so")
CFLAGS = ["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC]


def test_header_declares_and_library_exports_rl_resize():
    src = open(HEADER).read()
    assert "int rl_resize(rl_ctx* ctx, uint64_t table_slots, rl_resize_info* info /* may be NULL */);" in src
    assert "#define RL_ABI_VERSION 8u" in src
    assert "rl_resize" in _lib.EXPORTS
    if not os.path.exists(LIB):
        from ratelimit_amd import build
        build.build()
    lib = C.CDLL(LIB)
    assert hasattr(lib, "rl_resize")
    lib.rl_abi_version.restype = C.c_uint32
    assert lib.rl_abi_version() == abi.ABI_VERSION == 8


def test_resize_info_matches_the_c_layout(tmp_path):
    exe = str(tmp_path / "resize_layout")
    subprocess.run(CFLAGS + [os.path.join(ROOT, "tests", "c_abi", "resize_layout.c"), "-o", exe], check=True,
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
    cls = abi.RlResizeInfo
    assert sizes == {"rl_resize_info": C.sizeof(cls)} and C.sizeof(cls) == 48
    mirror = [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]
    assert mirror == fields["rl_resize_info"]  # the same fields in the same order, offsets and sizes
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION}


class _StubLib:
    """rl_resize as the library would answer it, recording what it was given."""

    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def rl_resize(self, ctx, table_slots, info_ref):
        self.calls.append((ctx, table_slots))
        if self.rc == abi.RL_OK:
            info = info_ref._obj
            info.slots_before, info.slots_after, info.keys = 1 << 10, table_slots, 700
            info.tombstones_dropped, info.log_entries_relinked, info.longest_probe = 24, 5, 3
        return self.rc

    def rl_last_error(self, ctx):
        return b"gpu: rl_resize: stub"


def _stub_backend(rc):
    be = Backend.__new__(Backend)  # (no rl_create: no device)
    be.L, be.ctx, be.cfg = _StubLib(rc), None, abi.RlConfig()
    be.cfg.table_slots = 1 << 10
    return be


def test_backend_resize_returns_the_info_and_tracks_the_size():
    be = _stub_backend(abi.RL_OK)
    got = be.resize(1 << 11)
    assert be.L.calls == [(None, 1 << 11)] and be.cfg.table_slots == 1 << 11
    assert got == {"slots_before": 1 << 10, "slots_after": 1 << 11, "keys": 700, "tombstones_dropped": 24,
                   "log_entries_relinked": 5, "longest_probe": 3}


def test_backend_resize_failure_raises_with_the_status_and_keeps_the_size():
    be = _stub_backend(abi.RL_E_TABLE_FULL)
    with pytest.raises(RedisError, match="RL_E_TABLE_FULL") as ei:
        be.resize(1 << 9)
    assert ei.value.status == abi.RL_E_TABLE_FULL and be.cfg.table_slots == 1 << 10
