"""CPU-side checks of the one-buffer request layout (rl_request_batch_packed,
rl_request_batch_pack) and of the pipelined entry point's declaration
(rl_do_limit_requests_packed_async): the header declares both functions and the
library exports them under ABI 8; the ctypes mirrors equal the C compiler's
layout field for field; the host converter round-trips request batches of every
shape the unpack kernel treats differently (a pure-Python decoder of the layout,
below, must give back every array of the input bytewise), follows the capacity
protocol, refuses malformed input without touching the buffer, and is clean
under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
(tests/c_abi/requests_packed_san.c)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import streams
from ratelimit_amd import abi, _lib
from ratelimit_amd.config import pack_requests
from ratelimit_amd.packing import RuleInterner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "ratelimit_hip.h")
LIB = os.path.join(ROOT, "ratelimit_amd", "libratelimit_hip.so")
CFLAGS = ["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
MIRROR = {"rl_request_override": abi.RlRequestOverride, "rl_request_batch_packed": abi.RlRequestBatchPacked}
TILE = abi.RL_REQUESTS_TILE
FILL = 0xA5


def library():
    if not os.path.exists(LIB):
        from ratelimit_amd import build
        build.build()
    return _lib.lib()


def test_header_declares_and_library_exports_the_packed_request_path():
    src = " ".join(open(HEADER).read().split())
    assert ("int rl_request_batch_pack(const rl_request_batch* in, uint8_t* buf, uint64_t buf_cap, "
            "rl_request_batch_packed* out);") in src
    assert ("int rl_do_limit_requests_packed_async(rl_ctx* ctx, const rl_request_batch_packed* in, "
            "rl_request_result* out, uint32_t opts, rl_request_verdict* verdict);") in src
    assert "#define RL_ABI_VERSION 8u" in src
    assert {"rl_request_batch_pack", "rl_do_limit_requests_packed_async"} <= set(_lib.EXPORTS)
    library()
    lib = C.CDLL(LIB)
    assert hasattr(lib, "rl_request_batch_pack") and hasattr(lib, "rl_do_limit_requests_packed_async")
    lib.rl_abi_version.restype = C.c_uint32
    assert lib.rl_abi_version() == abi.ABI_VERSION == 8


def test_packed_request_structs_match_the_c_layout(tmp_path):
    exe = str(tmp_path / "requests_packed_layout")
    subprocess.run(CFLAGS + [os.path.join(ROOT, "tests", "c_abi", "requests_packed_layout.c"), "-o", exe], check=True,
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
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION, "RL_REQUESTS_TILE": abi.RL_REQUESTS_TILE,
                      "RL_REQUESTS_INFLIGHT": abi.RL_REQUESTS_INFLIGHT}
    assert C.sizeof(abi.RlRequestOverride) == 16 and C.sizeof(abi.RlRequestBatchPacked) == 24 + 8 + 8 + 10 * 8


# ---- the converter --------------------------------------------------------------

def batch_struct(a, n_rules=5):
    b = abi.RlRequestBatch()
    b.n_requests, b.n_descriptors, b.n_entries, b.n_rules = len(a["hits"]), len(a["req_idx"]), len(a["key_len"]), \
        n_rules
    for k in abi.REQUEST_ARRAYS:
        setattr(b, k, abi.ptr(a[k]))
    return b


def pack(a, cap=None, n_rules=5):
    """-> (rc, RlRequestBatchPacked, the buffer). cap None: the size the converter asks for."""
    L = library()
    b = batch_struct(a, n_rules)
    p = abi.RlRequestBatchPacked()
    if cap is None:
        rc = L.rl_request_batch_pack(C.byref(b), None, 0, C.byref(p))
        if rc != abi.RL_E_CAPACITY:
            return rc, p, None
        cap = int(p.buf_bytes)
    buf = np.full(max(cap, 1), FILL, np.uint8)
    rc = L.rl_request_batch_pack(C.byref(b), abi.ptr(buf), cap, C.byref(p))
    return rc, p, buf


def decode(p, buf):
    """The packed layout -> the arrays of the rl_request_batch it came from
    (written from the header's description alone)."""
    nq, n, ne, nov = p.n_requests, p.n_descriptors, p.n_entries, p.n_overrides
    raw = bytes(buf[:p.buf_bytes])

    def sect(off, dtype, count):
        assert off % 4 == 0 and off + count * np.dtype(dtype).itemsize <= len(raw)
        return np.frombuffer(raw, dtype, count, off)

    req = sect(p.req, np.uint32, nq)
    nd, dl = (req & 0xFFFF).astype(np.int64), (req >> 16).astype(np.int64)
    cnt = sect(p.desc, np.uint16, n).astype(np.int64)
    kl, vl = sect(p.key_len, np.uint16, ne), sect(p.value_len, np.uint16, ne)
    a = {"now": sect(p.now, np.uint32, nq).astype(np.int64), "hits": sect(p.hits, np.uint32, nq).copy(),
         "key_len": kl.copy(), "value_len": vl.copy()}
    a["domain_off"] = np.concatenate([[0], np.cumsum(dl)]).astype(np.uint32)
    a["req_idx"] = np.repeat(np.arange(nq, dtype=np.uint32), nd)
    assert len(a["req_idx"]) == n and cnt.sum() == ne
    a["entry_first"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    ebytes = np.concatenate([[0], np.cumsum(kl.astype(np.int64) + vl + 2)])
    a["desc_off"] = ebytes[a["entry_first"]].astype(np.uint32)
    a["domain_bytes"] = sect(p.domain_bytes, np.uint8, int(a["domain_off"][-1])).copy()
    a["desc_bytes"] = sect(p.entry_bytes, np.uint8, int(a["desc_off"][-1])).copy()
    ov = sect(p.overrides, np.uint8, 16 * nov).reshape(nov, 16)
    a["override_flags"], a["override_unit"] = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    a["override_rpu"], a["override_rule"] = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    w = ov[:, :12].copy().view(np.uint32).reshape(nov, 3)
    assert (np.diff(w[:, 0].astype(np.int64)) > 0).all() and (w[:, 0] < max(n, 1)).all() and not ov[:, 13:].any()
    a["override_flags"][w[:, 0]] = 1
    a["override_rpu"][w[:, 0]], a["override_rule"][w[:, 0]], a["override_unit"][w[:, 0]] = w[:, 1], w[:, 2], ov[:, 12]
    # the tile index: entry t = the offsets of request t x TILE, the last the totals
    tiles = (nq + TILE - 1) // TILE
    index = sect(p.index, np.uint32, 4 * (tiles + 1)).reshape(tiles + 1, 4)
    first_desc = np.concatenate([[0], np.cumsum(nd)])
    for t in range(tiles + 1):
        q = min(t * TILE, nq)
        d = int(first_desc[q])
        assert list(index[t]) == [d, a["entry_first"][d], a["domain_off"][q], a["desc_off"][d]], t
    return a


def assert_roundtrip(a, n_rules=5):
    rc, p, buf = pack(a, None, n_rules)
    assert rc == abi.RL_OK
    n = len(a["req_idx"])
    assert (p.n_requests, p.n_descriptors, p.n_entries, p.n_rules) == (len(a["hits"]), n, len(a["key_len"]), n_rules)
    assert p.reserved == 0 and p.buf == buf.ctypes.data and p.buf_bytes == len(buf)
    got = decode(p, buf)
    for k in abi.REQUEST_ARRAYS:
        want = a[k]
        if want is None:  # no overrides: the dense arrays decode to zeros
            want = np.zeros(n, abi.REQUEST_DTYPES[k])
            assert p.n_overrides == 0
        elif k == "domain_bytes":
            want = want[:a["domain_off"][-1]]
        elif k == "desc_bytes":
            want = want[:a["desc_off"][-1]]
        assert got[k].dtype == abi.REQUEST_DTYPES[k] and got[k].tobytes() == np.ascontiguousarray(want).tobytes(), k
    return p, buf


def synthetic(descs_per_request, entries=None, overrides=(), seed=0):
    """rl_request_batch arrays with the given descriptors per request; ``entries``
    (descriptor -> entry count) defaults to 0-3 at random."""
    rng = np.random.default_rng(seed)
    nd = np.asarray(descs_per_request, np.int64)
    nq, n = len(nd), int(nd.sum())
    cnt = rng.integers(0, 4, n) if entries is None else np.array([entries(d) for d in range(n)], np.int64)
    ne = int(cnt.sum())
    kl, vl = rng.integers(0, 9, ne).astype(np.uint16), rng.integers(0, 7, ne).astype(np.uint16)
    ebytes = np.concatenate([[0], np.cumsum(kl.astype(np.int64) + vl + 2)])
    ent = np.concatenate([[0], np.cumsum(cnt)])
    dom_off = np.concatenate([[0], np.cumsum(rng.integers(0, 12, nq))])
    a = {"domain_bytes": rng.integers(97, 123, max(int(dom_off[-1]), 1)).astype(np.uint8),
         "domain_off": dom_off.astype(np.uint32), "now": (1_700_000_000 + np.arange(nq)).astype(np.int64),
         "hits": rng.integers(0, 9, nq).astype(np.uint32), "req_idx": np.repeat(np.arange(nq), nd).astype(np.uint32),
         "entry_first": ent.astype(np.uint32), "desc_off": ebytes[ent].astype(np.uint32),
         "desc_bytes": rng.integers(65, 91, max(int(ebytes[-1]), 1)).astype(np.uint8), "key_len": kl, "value_len": vl,
         "override_flags": None, "override_rpu": None, "override_unit": None, "override_rule": None}
    if len(overrides):
        ov = np.asarray(overrides, np.int64)
        a["override_flags"], a["override_unit"] = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        a["override_rpu"], a["override_rule"] = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        a["override_flags"][ov] = 1
        a["override_unit"][ov] = 1 + ov % 4
        a["override_rpu"][ov] = ov * 3 + 1
        a["override_rule"][ov] = ov % 5
    return a


@pytest.mark.parametrize("seed", [1, 2])
def test_pack_roundtrips_the_c4_streams(seed):
    calls = streams.c4_stream(seed, 1500, p_override=0.03)
    it = RuleInterner()
    for i in range(0, len(calls), 400):
        part = calls[i:i + 400]
        a = pack_requests([c[0] for c in part], [c[2] for c in part], it)
        assert_roundtrip(a, max(len(it.keys), 1))


@pytest.mark.parametrize("nq", [0, 1, 255, 256, 257, 513])
def test_pack_roundtrips_request_counts_around_the_tile(nq):
    rng = np.random.default_rng(nq)
    assert_roundtrip(synthetic(rng.integers(0, 4, nq), seed=nq))


def test_pack_roundtrips_the_edge_shapes():
    assert_roundtrip(synthetic([]))                              # the empty batch
    assert_roundtrip(synthetic([0, 0, 0]))                       # requests with 0 descriptors only
    assert_roundtrip(synthetic([0, 2, 0, 0, 3, 0]))              # ... at both ends and in the middle
    assert_roundtrip(synthetic([2, 1], entries=lambda d: 0))     # descriptors with 0 entries
    assert_roundtrip(synthetic([2, 3], entries=lambda d: 0 if d == 2 else 2))
    nd = [1] * 100 + [300] + [1] * 200                           # a request of 300 descriptors across a tile's chunk
    assert_roundtrip(synthetic(nd, seed=3))
    # overrides on the first and the last descriptor of a tile (tile 1 = requests 256..511, 2 descriptors each)
    nd = [2] * 600
    p, _ = assert_roundtrip(synthetic(nd, overrides=[512, 1023], seed=4))
    assert p.n_overrides == 2
    p, _ = assert_roundtrip(synthetic(nd, overrides=[0, 511, 512, 1023, 1199], seed=5))
    assert p.n_overrides == 5
    a = synthetic([3, 3], overrides=[1], seed=6)
    a["override_flags"][4] = 2  # only bit 0 means "present"
    rc, p, buf = pack(a)
    assert rc == abi.RL_OK and p.n_overrides == 1


def test_pack_capacity_protocol():
    a = synthetic([2] * 300, overrides=[5], seed=7)
    L = library()
    b = batch_struct(a)
    p = abi.RlRequestBatchPacked()
    assert L.rl_request_batch_pack(C.byref(b), None, 0, C.byref(p)) == abi.RL_E_CAPACITY
    need = int(p.buf_bytes)
    assert need % 4 == 0 and need >= 16 * 3
    assert (p.n_requests, p.buf) == (0, None)  # nothing else written
    for cap in (0, 1, need // 2, need - 1):
        rc, p, buf = pack(a, cap)
        assert rc == abi.RL_E_CAPACITY and p.buf_bytes == need and (buf == FILL).all()
    rc, p, buf = pack(a, need)
    assert rc == abi.RL_OK and p.buf_bytes == need
    rc, p, big = pack(a, need + 64)  # a larger buffer: the same bytes, the rest untouched
    assert rc == abi.RL_OK and p.buf_bytes == need and big[:need].tobytes() == buf[:need].tobytes()
    assert (big[need:] == FILL).all()


def bad_batches():
    def fresh():
        return synthetic([2] * 300, overrides=[5], seed=8)

    a = fresh()
    a["domain_off"][5] = a["domain_off"][6] + 1
    yield "domain_off not monotone", a
    a = fresh()
    a["domain_off"][0] = 1
    yield "domain_off does not start at 0", a
    a = fresh()
    a["entry_first"][9] = a["entry_first"][10] + 1
    yield "entry_first not monotone", a
    a = fresh()
    a["entry_first"][-1] += 1
    yield "entry_first does not end at n_entries", a
    a = fresh()
    a["desc_off"][-1] += 1
    yield "a desc_off span that is not its entries' sum", a
    a = fresh()
    a["key_len"][3] += 1
    yield "an entry length that does not tile the span", a
    a = fresh()
    a["desc_off"][9], a["desc_off"][10] = a["desc_off"][10], a["desc_off"][9] - 1
    yield "desc_off not monotone", a
    a = fresh()
    a["req_idx"][20] = 300
    yield "req_idx >= n_requests", a
    a = fresh()
    a["req_idx"][20] = 3
    yield "req_idx decreasing", a
    a = fresh()
    a["now"][3] = -1
    yield "now negative", a
    a = fresh()
    a["now"][3] = 1 << 32
    yield "now past 32 bits", a
    a = fresh()
    a["override_rule"] = None
    yield "override_flags without override_rule", a
    yield "a request of 65536 descriptors", synthetic([1, 65536, 1], entries=lambda d: 0)
    a = synthetic([1])
    a["domain_off"][1] = 65536
    a["domain_bytes"] = np.zeros(65536, np.uint8)
    yield "a domain of 65536 bytes", a
    a = synthetic([1], entries=lambda d: 65536)
    yield "a descriptor of 65536 entries", a


@pytest.mark.parametrize("name,a", list(bad_batches()), ids=[n for n, _ in bad_batches()])
def test_pack_refuses_malformed_batches_and_writes_nothing(name, a):
    rc, p, buf = pack(a, 1 << 21)
    assert rc == abi.RL_E_INVALID, name
    assert (buf == FILL).all()
    assert pack(a)[0] == abi.RL_E_INVALID  # the sizing call refuses it too


def test_pack_accepts_the_largest_counts():
    assert_roundtrip(synthetic([1, 65535, 1], entries=lambda d: 0))
    assert_roundtrip(synthetic([1], entries=lambda d: 65535))
    a = synthetic([1])
    a["domain_off"][1] = 65535
    a["domain_bytes"] = np.full(65535, 100, np.uint8)
    assert_roundtrip(a)


def test_converter_is_clean_under_asan_and_ubsan(tmp_path):
    """The converter and a stand-alone driver, both instrumented: well-formed
    batches, every truncated capacity, the malformed inputs above."""
    if not shutil.which("gcc") or not shutil.which("g++"):
        pytest.skip("no gcc")
    objs = []
    for src, cc, std in ((os.path.join(ROOT, "ratelimit_amd", "csrc", "rl_pack.cpp"), "g++", "-std=c++17"),
                         (os.path.join(ROOT, "tests", "c_abi", "requests_packed_san.c"), "gcc", "-std=c11")):
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cc, std, "-I" + INC, "-Wall", "-c", src, "-o", o] + SAN, check=True, capture_output=True,
                       text=True)
        objs.append(o)
    exe = str(tmp_path / "requests_packed_san")
    subprocess.run(["g++", "-o", exe] + objs + SAN, check=True, capture_output=True, text=True)
    syms = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    assert "__asan_report_load" in syms and "__ubsan_handle" in syms  # (instrumented)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("OK ") and int(r.stdout.split()[1]) > 300
