"""CPU-side checks of rl_scan: the header declares it and the library exports it
under ABI 8 (symbols and types only added); the ctypes mirrors of
rl_scan_query / rl_scan_cursor / rl_scan_prefix_sum / rl_scan_info equal the C
compiler's layout of include/ratelimit_hip.h field for field
(tests/c_abi/scan_layout.c); the page planner rl_scan_plan.h, compiled for the
host plain and under AddressSanitizer + UndefinedBehaviorSanitizer as a
stand-alone program, agrees with a brute-force loop
(tests/c_abi/scan_plan_run.cpp); Backend.scan / count_keys pass flags, masks,
offsets and cursors through, walk the shards, retry once on RL_E_CAPACITY with
need_* and raise with the status otherwise (a stub library: no device);
list_keys builds forget_domain's prefix; and the stream the GPU tests run has,
under the prefixes they use, every kind of key (the oracle alone)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from ratelimit_amd import abi, _lib
from ratelimit_amd.limiter import Backend, FixedTimeSource, GpuRateLimitCache, RedisError
from ratelimit_amd.packing import stem_of
import scan_cases as SC
from test_gpu_forget import DIV, fg_stream, seen_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "ratelimit_hip.h")
LIB = os.path.join(ROOT, "ratelimit_amd", "libratelimit_hip.so")
CFLAGS = ["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]

MIRROR = {"rl_scan_query": abi.RlScanQuery, "rl_scan_cursor": abi.RlScanCursor,
          "rl_scan_prefix_sum": abi.RlScanPrefixSum, "rl_scan_info": abi.RlScanInfo}


def test_header_declares_and_library_exports_rl_scan():
    src = open(HEADER).read()
    assert ("int rl_scan(rl_ctx* ctx, const rl_scan_query* q, rl_scan_cursor* cur /* in, out */,\n"
            "            rl_records* out /* NULL: count only */, rl_scan_prefix_sum* by_prefix "
            "/* [max(n_prefixes, 1)] or NULL */,\n"
            "            rl_scan_info* info /* may be NULL */);") in src
    assert "#define RL_ABI_VERSION 8u" in src
    assert "rl_scan" in _lib.EXPORTS
    if not os.path.exists(LIB):
        from ratelimit_amd import build
        build.build()
    lib = C.CDLL(LIB)
    assert hasattr(lib, "rl_scan")
    lib.rl_abi_version.restype = C.c_uint32
    assert lib.rl_abi_version() == abi.ABI_VERSION == 8


def test_scan_structs_match_the_c_layout(tmp_path):
    exe = str(tmp_path / "scan_layout")
    subprocess.run(CFLAGS + [os.path.join(ROOT, "tests", "c_abi", "scan_layout.c"), "-o", exe], check=True,
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
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION, "RL_SCAN_NEWEST": abi.RL_SCAN_NEWEST,
                      "RL_SCAN_LIVE": abi.RL_SCAN_LIVE, "RL_SCAN_TILE": abi.RL_SCAN_TILE}
    assert (abi.RL_SCAN_NEWEST, abi.RL_SCAN_LIVE, abi.RL_SCAN_TILE) == (1, 2, 1024)


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_scan_planner_on_the_host(tmp_path, flags):
    """rlscan::plan against a brute-force loop: no tiles; the first tile not
    fitting; an exact fit and one short of it; the record cap binding before
    the byte cap and the reverse; the 2^32 byte bound; a short last tile; 4000
    random tile lists. Each tile's base is the sum of the tiles before it and
    nothing is written past the cut."""
    assert shutil.which("g++"), "the host build of rl_scan_plan.h needs g++"
    exe = str(tmp_path / "scan_plan_run")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "ratelimit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_abi", "scan_plan_run.cpp"), "-o", exe] + flags, check=True,
                   capture_output=True, text=True)
    if flags is SAN:
        syms = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
        assert "__asan_" in syms and "__ubsan_handle" in syms  # (instrumented)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) >= 4020


# --------------------------------------------------------------------------- the wrappers over a stub library
class _StubLib:
    """rl_scan as the library would answer it over shards of `tiles` tiles with
    `per_tile` records of 10-byte stems each, recording what it was given. A
    page covers the tiles that fit, as the library's planner would cut."""

    def __init__(self, rc=abi.RL_OK, n_shards=1, tiles=3, per_tile=5):
        self.rc, self.n_shards, self.tiles, self.per_tile, self.calls = rc, n_shards, tiles, per_tile, []

    def rl_scan(self, ctx, qref, cref, rref, byp, iref):
        q, cur, info = qref._obj, cref._obj, iref._obj
        off = np.ctypeslib.as_array(C.cast(q.prefix_off, C.POINTER(C.c_uint32)), (q.n_prefixes + 1,)).copy()
        blob = bytes(np.ctypeslib.as_array(C.cast(q.prefix_bytes, C.POINTER(C.c_uint8)), (max(int(off[-1]), 1),)))
        r = rref._obj if rref is not None else None
        self.calls.append({"ctx": ctx, "flags": q.flags, "now": q.now, "unit_mask": q.unit_mask, "off": off.tolist(),
                           "reserved": (q.reserved, cur.reserved),
                           "prefixes": [blob[off[i]:off[i + 1]] for i in range(q.n_prefixes)],
                           "cursor": (cur.shard, cur.slot), "cap": None if r is None else (r.n, r.stem_cap)})
        if self.rc != abi.RL_OK:
            return self.rc
        assert cur.shard < self.n_shards and cur.slot % abi.RL_SCAN_TILE == 0
        first = cur.slot // abi.RL_SCAN_TILE
        left = self.tiles - first
        if r is None:
            k = left
        else:
            k = min(left, r.n // self.per_tile, r.stem_cap // (10 * self.per_tile))
            if k == 0:
                info.need_records, info.need_stem_bytes = self.per_tile, 10 * self.per_tile
                return abi.RL_E_CAPACITY
            n = k * self.per_tile
            r.n = n
            so = np.ctypeslib.as_array(C.cast(r.stem_off, C.POINTER(C.c_uint32)), (n + 1,))
            so[:] = np.arange(n + 1) * 10
            ws = np.ctypeslib.as_array(C.cast(r.ws, C.POINTER(C.c_uint32)), (n,))
            ws[:] = (cur.shard * 1000 + first * 100) + np.arange(n)
        info.slots_scanned, info.keys, info.records = k * abi.RL_SCAN_TILE, k * self.per_tile, k * self.per_tile
        info.stem_bytes, info.time_floor = 10 * k * self.per_tile, 7
        nb = max(q.n_prefixes, 1)
        np.ctypeslib.as_array(C.cast(byp, C.POINTER(C.c_uint64)), (nb, 3))[:] = [[k, k * self.per_tile, 3 * k]] * nb
        if first + k == self.tiles:
            cur.shard, cur.slot = cur.shard + 1, 0
        else:
            cur.slot = (first + k) * abi.RL_SCAN_TILE
        return abi.RL_OK

    def rl_last_error(self, ctx):
        return b"gpu: rl_scan: stub"


def _stub_backend(**kw):
    n_shards = kw.get("n_shards", 1)
    be = Backend.__new__(Backend)  # (no rl_create: no device)
    be.L, be.ctx, be.cfg = _StubLib(**kw), None, abi.RlConfig()
    be.cfg.max_batch, be.cfg.max_stem_bytes, be.cfg.n_shards = 1 << 12, 1 << 16, n_shards
    return be


def test_backend_scan_passes_the_query_through_and_walks_pages_and_shards():
    be = _stub_backend(n_shards=2)
    pages = list(be.scan([b"dom_a_", b"dom_b_x"], units=[1, 4], now=1234, newest=True, page_records=10,
                         page_stem_bytes=1000))
    calls = be.L.calls
    assert [c["cursor"] for c in calls] == [(0, 0), (0, 2048), (1, 0), (1, 2048)]
    for c in calls:
        assert c["flags"] == abi.RL_SCAN_NEWEST | abi.RL_SCAN_LIVE and c["now"] == 1234
        assert c["unit_mask"] == (1 << 1) | (1 << 4) and c["reserved"] == (0, 0)
        assert c["prefixes"] == [b"dom_a_", b"dom_b_x"] and c["off"] == [0, 6, 13] and c["cap"] == (10, 1000)
    assert [len(rec["ws"]) for rec, _, _ in pages] == [10, 5, 10, 5]
    assert [int(rec["ws"][0]) for rec, _, _ in pages] == [0, 200, 1000, 1200]
    assert [len(rec["stem_off"]) for rec, _, _ in pages] == [11, 6, 11, 6]
    assert [d["shard"] for _, d, _ in pages] == [0, 0, 1, 1]
    assert [d["cursor"] for _, d, _ in pages] == [(0, 2048), (1, 0), (1, 2048), (2, 0)]
    assert pages[0][1]["records"] == 10 and pages[0][1]["time_floor"] == 7
    assert pages[0][2].shape == (2, 3) and pages[0][2].dtype == np.uint64 and pages[0][2].tolist() == [[2, 10, 6]] * 2
    # the defaults: no prefix (every key), no mask, no flags, 64 stem bytes per record
    be = _stub_backend()
    (page,) = list(be.scan())
    (c,) = be.L.calls
    assert c["flags"] == 0 and c["unit_mask"] == 0 and c["prefixes"] == [] and c["off"] == [0]
    assert c["cap"] == (1 << 16, 64 << 16) and page[2].shape == (1, 3) and len(page[0]["ws"]) == 15
    list(be.scan(newest=True))
    assert be.L.calls[-1]["flags"] == abi.RL_SCAN_NEWEST
    list(be.scan(now=0))  # (a clock of 0 is a clock)
    assert be.L.calls[-1]["flags"] == abi.RL_SCAN_LIVE and be.L.calls[-1]["now"] == 0


def test_backend_scan_retries_once_on_capacity_with_need():
    be = _stub_backend(n_shards=2, tiles=2, per_tile=5)
    pages = list(be.scan([b"p"], page_records=3, page_stem_bytes=20))
    caps = [(c["cursor"], c["cap"]) for c in be.L.calls]
    # the first page asks again with need_*; the later pages keep the grown buffers
    assert caps == [((0, 0), (3, 20)), ((0, 0), (5, 50)), ((0, 1024), (5, 50)), ((1, 0), (5, 50)), ((1, 1024), (5, 50))]
    assert [len(rec["ws"]) for rec, _, _ in pages] == [5, 5, 5, 5]

    class Stuck(_StubLib):  # still too small after the retry: the second RL_E_CAPACITY is raised
        def rl_scan(self, *a):
            rc = super().rl_scan(*a)
            a[5]._obj.need_records = 1 << 20
            return abi.RL_E_CAPACITY if len(self.calls) <= 2 else rc

    be = _stub_backend()
    be.L = Stuck()
    with pytest.raises(RedisError, match="RL_E_CAPACITY") as ei:
        list(be.scan(page_records=3))
    assert ei.value.status == abi.RL_E_CAPACITY and len(be.L.calls) == 2


def test_backend_scan_failure_raises_with_the_status():
    for rc, name in ((abi.RL_E_INVALID, "RL_E_INVALID"), (abi.RL_E_TIME, "RL_E_TIME"), (abi.RL_E_HIP, "RL_E_HIP")):
        be = _stub_backend(rc=rc)
        with pytest.raises(RedisError, match=name) as ei:
            list(be.scan([b"x"], now=5))
        assert ei.value.status == rc and "stub" in str(ei.value) and len(be.L.calls) == 1
        with pytest.raises(RedisError, match=name):
            be.count_keys([b"x"])
    be = _stub_backend(rc=abi.RL_E_CAPACITY)  # (no need_*: the prefixes are too many; not retried)
    with pytest.raises(RedisError, match="RL_E_CAPACITY"):
        list(be.scan([b"x"] * 65))
    assert len(be.L.calls) == 1 and len(be.L.calls[0]["prefixes"]) == 65


def test_backend_count_keys_sums_over_the_shards():
    be = _stub_backend(n_shards=3, tiles=4, per_tile=2)
    got = be.count_keys([b"a_", b"b_"], units=[2], now=99, newest=True)
    assert [c["cursor"] for c in be.L.calls] == [(0, 0), (1, 0), (2, 0)]
    assert all(c["cap"] is None and c["unit_mask"] == 4 and c["flags"] == 3 and c["now"] == 99 for c in be.L.calls)
    assert {k: v for k, v in got.items() if k != "by_prefix"} == {
        "slots_scanned": 3 * 4096, "keys": 24, "records": 24, "stem_bytes": 240, "chains_lost": 0}
    assert got["by_prefix"].tolist() == [[12, 24, 36]] * 2


def test_cache_list_keys_builds_the_prefix_of_forget_domain():
    cache = GpuRateLimitCache.__new__(GpuRateLimitCache)
    cache.prefix = "pfx:"
    cache.time_source = FixedTimeSource(4321)
    cache.backend = _stub_backend()
    got = cache.list_keys("dom")
    c = cache.backend.L.calls[-1]
    # (the prefix forget_domain builds: tests/test_forget_cpu.py)
    assert c["prefixes"] == [b"pfx:dom_"] == [("pfx:" + "dom" + "_").encode()]
    assert c["flags"] == abi.RL_SCAN_NEWEST | abi.RL_SCAN_LIVE and c["now"] == 4321 and c["unit_mask"] == 0
    assert len(got) == 15 and got[0].stem == b"\0" * 10 and [k.ws for k in got[:3]] == [0, 1, 2]
    cache.list_keys("dom", live=False, newest=False)
    assert cache.backend.L.calls[-1]["flags"] == 0
    cache.list_keys("dom", entries=[("k", "v")])
    assert cache.backend.L.calls[-1]["prefixes"] == [stem_of("pfx:", "dom", [("k", "v")])] == [b"pfx:dom_k_v_"]


# --------------------------------------------------------------------------- the GPU tests' stream, the oracle alone
@pytest.mark.parametrize("local_cache,per_second", [(False, False), (True, False), (False, True), (True, True)])
def test_scan_stream_has_every_case(local_cache, per_second):
    """The first half of fg_stream(5) under the prefixes the GPU tests use
    (SC.DOMAIN, SC.p64()): stems under two units, stems longer than 36 bytes,
    keys with a history chain, records already expired at the scan's clock T and
    records still live, stems in two domains of which one's name begins the
    other's. Of each kind the 64 prefixes select some and leave some; the domain
    prefix selects some of each kind and leaves the other domain."""
    calls = fg_stream(5)
    half = len(calls) // 2
    oc = O.OracleFixedRateLimitCache(0.8, local_cache, per_second=per_second)
    for r, l, now in calls[:half]:
        oc.do_limit(r, l, now)
    T = calls[half][2]
    seen = seen_keys(calls[:half])
    stores = [oc.client] + ([oc.per_second_client] if per_second else [])
    keys = {k: e for s in stores for k, e in s.data.items()}
    assert keys and all(e[1] >= 0 for e in keys.values())
    kinds = {
        "two_units": {s for s in seen if len(seen[s]) >= 2},
        "long": {s for s in seen if len(s) > 36},
        # a slot has a chain once its newest window moved while the older one was within 8 windows of it
        "history": {s for s in seen for u, ws in seen[s].items() if any(0 < a - b <= 8 * DIV[u] for a in ws for b in ws)},
        "expired": {k.rstrip("0123456789").encode() for k, e in keys.items() if T > e[1]},
        "live": {k.rstrip("0123456789").encode() for k, e in keys.items() if T <= e[1]},
        "domain_fg": {s for s in seen if s.startswith(b"fg_stem_")},
        "domain_fg_b": {s for s in seen if s.startswith(b"fg_b_stem_")},
    }
    assert kinds["domain_fg"] | kinds["domain_fg_b"] == set(seen)  # "fg_" begins both domains' stems
    assert all(s.startswith(SC.BOTH[0]) for s in seen)
    for name, prefixes in (("domain", SC.DOMAIN), ("p64", SC.p64())):
        sel = {s for s in seen if any(s.startswith(p) for p in prefixes)}
        for kind, stems in kinds.items():
            if name == "p64":  # of each kind some, and some left
                assert stems & sel and stems - sel, (name, kind, len(stems), len(stems & sel))
            elif kind != "domain_fg_b":  # the one domain: some of each kind (all its stems under two units are there)
                assert stems & sel, (name, kind)
        assert sel and set(seen) - sel
    assert kinds["domain_fg"] == {s for s in seen if s.startswith(SC.DOMAIN[0])} != set(seen)
    # p64's special entries do what their comments say
    p = SC.p64()
    assert p[0] in seen and p[1][:-1] in seen and not any(s.startswith(p[1]) for s in seen)
    assert any(s.startswith(p[2]) and s != p[0] for s in seen) and any(s.startswith(p[3]) for s in seen)
    assert any(s.startswith(p[7]) for s in seen) and not any(s.startswith(p[8]) for s in seen)
    assert all(len(x) > 36 for x in seen if x.startswith(p[7])) and len(p[7]) > 36
    edge = SC.edge_stems()
    assert sorted(len(x) for x in p[11:15]) == [32, 33, 36, 37] and sorted(len(x) for x in p[15:19]) == [1, 3, 4, 5]
    for q in p[9:19]:
        assert any(s.startswith(q) for s in edge), q
    assert not all(any(s.startswith(q) for q in p) for s in edge)
