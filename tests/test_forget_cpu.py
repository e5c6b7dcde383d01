"""CPU-side checks of rl_forget: the header declares it and the library exports
it under ABI 8 (symbols and types only added); the ctypes mirrors of rl_stems /
rl_forget_info equal the C compiler's layout of include/ratelimit_hip.h field
for field (tests/c_abi/forget_layout.c); Backend.forget passes flags and offsets
through, returns the info's fields and raises with the status (a stub library:
no device); the cache builds peek's stems and the domain prefix;
rl_forget_match.h, compiled for the host plain and under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program, agrees with memcmp over
the slot's "inline bytes + arena" layout (tests/c_abi/forget_match_run.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from ratelimit_amd import abi, _lib
from ratelimit_amd.limiter import Backend, GpuRateLimitCache, RedisError
from ratelimit_amd.packing import stem_of
from ratelimit_amd.types import Descriptor, RateLimitRequest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "ratelimit_hip.h")
LIB = os.path.join(ROOT, "ratelimit_amd", "libratelimit_hip.so")
CFLAGS = ["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]

MIRROR = {"rl_stems": abi.RlStems, "rl_forget_info": abi.RlForgetInfo}


def test_header_declares_and_library_exports_rl_forget():
    src = open(HEADER).read()
    assert ("int rl_forget(rl_ctx* ctx, const rl_stems* in, uint32_t* removed /* [n] or NULL */,\n"
            "              rl_forget_info* info /* may be NULL */);") in src
    assert "#define RL_ABI_VERSION 8u" in src
    assert "rl_forget" in _lib.EXPORTS
    if not os.path.exists(LIB):
        from ratelimit_amd import build
        build.build()
    lib = C.CDLL(LIB)
    assert hasattr(lib, "rl_forget")
    lib.rl_abi_version.restype = C.c_uint32
    assert lib.rl_abi_version() == abi.ABI_VERSION == 8


def test_forget_structs_match_the_c_layout(tmp_path):
    exe = str(tmp_path / "forget_layout")
    subprocess.run(CFLAGS + [os.path.join(ROOT, "tests", "c_abi", "forget_layout.c"), "-o", exe], check=True,
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
    assert C.sizeof(abi.RlForgetInfo) == 32
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION, "RL_FORGET_PREFIX": abi.RL_FORGET_PREFIX,
                      "RL_FORGET_DRY_RUN": abi.RL_FORGET_DRY_RUN, "RL_FORGET_PREFIX_MAX": abi.RL_FORGET_PREFIX_MAX,
                      "RL_FORGET_PREFIX_BYTES": abi.RL_FORGET_PREFIX_BYTES}
    assert (abi.RL_FORGET_PREFIX, abi.RL_FORGET_DRY_RUN, abi.RL_FORGET_PREFIX_MAX, abi.RL_FORGET_PREFIX_BYTES) == \
        (1, 2, 64, 4096)


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_forget_match_header_on_the_host(tmp_path, flags):
    """begins_with / head_may_match against memcmp: stems of 1, 3, 4, 5, 31, 32,
    33, 36, 37, 47, 48, 49 and 200 bytes stored as slots store them, prefixes of
    1..40, 48, 49 and 200 bytes (equal to the stem, one byte longer, differing
    in the last byte only, in the first, at each layout edge)."""
    assert shutil.which("g++"), "the host build of rl_forget_match.h needs g++"
    exe = str(tmp_path / "forget_match_run")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "ratelimit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_abi", "forget_match_run.cpp"), "-o", exe] + flags, check=True,
                   capture_output=True, text=True)
    if flags is SAN:
        syms = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
        assert "__asan_" in syms and "__ubsan_handle" in syms  # (instrumented)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout
    # 13 stems x 43 prefix lengths x (the prefix itself, its last and its first byte changed) at the least
    assert int(r.stdout.split()[1]) >= 13 * 43 * 3


class _StubLib:
    """rl_forget as the library would answer it, recording what it was given:
    every entry removes (its length mod 5) slots."""

    def __init__(self, rc=abi.RL_OK):
        self.rc, self.calls = rc, []

    def rl_forget(self, ctx, sref, removed, iref):
        s, info = sref._obj, iref._obj
        off = np.ctypeslib.as_array(C.cast(s.stem_off, C.POINTER(C.c_uint32)), (s.n + 1,)).copy()
        blob = bytes(np.ctypeslib.as_array(C.cast(s.stem_bytes, C.POINTER(C.c_uint8)), (max(int(off[-1]), 1),)))
        self.calls.append({"ctx": ctx, "n": s.n, "flags": s.flags, "off": off.tolist(),
                           "stems": [blob[off[i]:off[i + 1]] for i in range(s.n)]})
        if self.rc != abi.RL_OK:
            return self.rc
        out = np.ctypeslib.as_array(C.cast(removed, C.POINTER(C.c_uint32)), (s.n,))
        out[:] = [(off[i + 1] - off[i]) % 5 for i in range(s.n)]
        info.slots_scanned = 1024 if s.flags & abi.RL_FORGET_PREFIX else 0
        info.keys, info.keys_with_history, info.arena_bytes = int(out.sum()), 1, 16 * s.n
        return abi.RL_OK

    def rl_last_error(self, ctx):
        return b"gpu: rl_forget: stub"


def _stub_backend(rc=abi.RL_OK, max_batch=1 << 12, max_stem_bytes=1 << 16):
    be = Backend.__new__(Backend)  # (no rl_create: no device)
    be.L, be.ctx, be.cfg = _StubLib(rc), None, abi.RlConfig()
    be.cfg.max_batch, be.cfg.max_stem_bytes, be.cfg.n_shards = max_batch, max_stem_bytes, 1
    return be


STEMS = [b"dom_k_v_", b"dom_kk_vv_", b"x" * 200 + b"_", b"d_a_b_c_d_"]


def test_backend_forget_passes_flags_and_offsets_and_returns_the_fields():
    be = _stub_backend()
    got = be.forget(STEMS)
    (call,) = be.L.calls
    assert call["n"] == 4 and call["flags"] == 0 and call["stems"] == STEMS
    assert call["off"] == [0, 8, 18, 219, 229]
    want = [len(s) % 5 for s in STEMS]
    assert got["removed"].dtype == np.uint32 and got["removed"].tolist() == want
    assert {k: v for k, v in got.items() if k != "removed"} == {
        "slots_scanned": 0, "keys": sum(want), "keys_with_history": 1, "arena_bytes": 64}
    for kw, flags in (({"prefix": True}, abi.RL_FORGET_PREFIX), ({"dry_run": True}, abi.RL_FORGET_DRY_RUN),
                      ({"prefix": True, "dry_run": True}, abi.RL_FORGET_PREFIX | abi.RL_FORGET_DRY_RUN)):
        got = be.forget(STEMS[:2], **kw)
        assert be.L.calls[-1]["flags"] == flags and be.L.calls[-1]["stems"] == STEMS[:2]
        assert got["slots_scanned"] == (1024 if kw.get("prefix") else 0)
    # nothing to forget: no call, zeros
    n_calls = len(be.L.calls)
    got = be.forget([])
    assert len(be.L.calls) == n_calls and len(got["removed"]) == 0 and got["keys"] == 0


def test_backend_forget_splits_keyed_stems_at_the_ctx_limits_and_sums():
    be = _stub_backend(max_batch=3, max_stem_bytes=64)
    stems = [b"s%02d_" % i for i in range(7)] + [b"y" * 60 + b"_", b"z_"]
    got = be.forget(stems)
    assert [c["n"] for c in be.L.calls] == [3, 3, 1, 2]  # (61 bytes alone: the next stem would pass 64)
    assert [s for c in be.L.calls for s in c["stems"]] == stems
    assert all(c["off"][0] == 0 for c in be.L.calls)
    assert got["removed"].tolist() == [len(s) % 5 for s in stems] and got["keys"] == int(got["removed"].sum())
    assert got["keys_with_history"] == 4 and got["arena_bytes"] == 16 * len(stems)
    # prefixes are one call whatever their number: the library answers RL_E_CAPACITY itself
    be = _stub_backend(max_batch=3)
    be.forget([b"p%02d" % i for i in range(65)], prefix=True)
    assert [c["n"] for c in be.L.calls] == [65]


def test_backend_forget_failure_raises_with_the_status():
    for rc, name in ((abi.RL_E_INVALID, "RL_E_INVALID"), (abi.RL_E_CAPACITY, "RL_E_CAPACITY")):
        be = _stub_backend(rc)
        with pytest.raises(RedisError, match=name) as ei:
            be.forget(STEMS, prefix=True)
        assert ei.value.status == rc and "stub" in str(ei.value)


def test_cache_forget_builds_the_stems_of_peek_and_the_domain_prefix():
    cache = GpuRateLimitCache.__new__(GpuRateLimitCache)
    cache.prefix = "pfx:"
    cache.backend = _stub_backend()
    req = RateLimitRequest("dom", [Descriptor([("k", "v")]), Descriptor([("a", "b"), ("c", "d")]),
                                   Descriptor([("k2", "v2")])], 1)
    lim = object()  # (only nil or not matters here)
    want = [stem_of("pfx:", "dom", d.entries) for d in req.descriptors]
    assert want[0] == b"pfx:dom_k_v_"
    cache.forget(req)
    assert cache.backend.L.calls[-1]["stems"] == want and cache.backend.L.calls[-1]["flags"] == 0
    cache.forget(req, [lim, None, lim], dry_run=True)  # a nil limit is left out, as do_limit leaves it
    assert cache.backend.L.calls[-1]["stems"] == [want[0], want[2]]
    assert cache.backend.L.calls[-1]["flags"] == abi.RL_FORGET_DRY_RUN
    with pytest.raises(AssertionError):
        cache.forget(req, [lim])
    got = cache.forget_domain("dom")
    assert cache.backend.L.calls[-1]["stems"] == [b"pfx:dom_"]
    assert cache.backend.L.calls[-1]["flags"] == abi.RL_FORGET_PREFIX and got["slots_scanned"] == 1024
    cache.forget_domain("dom", dry_run=True)
    assert cache.backend.L.calls[-1]["flags"] == abi.RL_FORGET_PREFIX | abi.RL_FORGET_DRY_RUN
