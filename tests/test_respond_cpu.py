"""The serialized responses on the CPU: the ABI additions (header, exports, the
ctypes mirrors against a C99 compiler's layout), the independent encoder
(tests/response_ref.py) against the committed fixture and the protobuf
runtime, the host twin rl_response_serialize against that encoder, the bound,
and the emitter the kernels share (ratelimit_amd/csrc/rl_resp_emit.h) run on
the host by tests/c_abi/resp_emit_run.cpp, plain and under AddressSanitizer +
UndefinedBehaviorSanitizer. No GPU call."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from ratelimit_amd import _lib, abi
from ratelimit_amd.limiter import Backend, RedisError
import response_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "ratelimit_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
GOLDEN = json.load(open(os.path.join(HERE, "golden", "response_wire.json")))
NEW = ["rl_response_bound", "rl_do_limit_wire_respond_async", "rl_response_serialize", "rl_debug_respond"]


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(INC, "ratelimit_hip.h")).read()
    assert "#define RL_ABI_VERSION 8u" in text
    L = _lib.lib()
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, text), f
        assert f in _lib.EXPORTS and hasattr(L, f), f
    assert L.rl_abi_version() == 8


def test_ctypes_mirrors_equal_the_c99_layout(tmp_path):
    exe = str(tmp_path / "respond_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC,
                    os.path.join(HERE, "c_abi", "respond_layout.c"), "-o", exe], check=True, capture_output=True,
                   text=True)
    sizes, fields, consts = {}, {}, {}
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n"):
        p = ln.split()
        if p and p[0] == "S":
            sizes[p[1]] = int(p[2])
        elif p and p[0] == "F":
            fields.setdefault(p[1], []).append((p[2], int(p[3]), int(p[4])))
        elif p and p[0] == "C":
            consts[p[1]] = int(p[2])
    mirror = {"rl_response_format": abi.RlResponseFormat, "rl_response_batch": abi.RlResponseBatch}
    assert set(sizes) == set(mirror)
    for name, cls in mirror.items():
        assert C.sizeof(cls) == sizes[name], name
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == fields[name], name
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION, "RL_RESPONSE_KEY_MAX": abi.RL_RESPONSE_KEY_MAX,
                      "RL_RESPONSE_STATUS_MAX": abi.RL_RESPONSE_STATUS_MAX, "RL_NO_DESCRIPTOR": abi.RL_NO_DESCRIPTOR,
                      "RL_MATCH_LIMIT": abi.RL_MATCH_LIMIT}
    assert (abi.RL_RESPONSE_KEY_MAX, abi.RL_RESPONSE_STATUS_MAX) == (R.KEY_MAX, R.STATUS_MAX) == (64, 26)


# ---- the independent encoder against the fixture and the protobuf runtime ----

def golden_cases():
    for c in GOLDEN["cases"]:
        keys = None if c["keys"] is None else tuple(bytes.fromhex(k) for k in c["keys"])
        yield [tuple(d) for d in c["descs"]], c["global_shadow"], keys, c


def test_reference_encoder_equals_the_fixture():
    n = 0
    for descs, gs, keys, c in golden_cases():
        code, headers = R.verdict_of(descs, gs)
        assert (code, None if headers is None else list(headers)) == (c["overall_code"], c["headers"])
        got = R.encode_request(descs, gs, keys)
        assert got.hex() == c["hex"], descs[:3]
        # and the decoder reads the same answers back
        dcode, sts, hdrs = R.decode_response(got)
        assert dcode == code
        assert sts == [(d[0], (d[2], d[3]) if d[1] == R.LIMIT else None, d[4], d[5] if d[1] == R.LIMIT else None)
                       for d in descs]
        want_h = [] if keys is None or headers is None else [(k, b"%d" % v) for k, v in zip(keys, headers)]
        assert hdrs == want_h
        n += 1
    assert 40 <= n <= 100
    # the fixture holds the three shapes the contract spells out
    hexes = {c["hex"] for c in GOLDEN["cases"]}
    assert "0801" in hexes and "080112020801" in hexes and "08011208080118ffffffff0f" in hexes
    assert len(R.encode_status(R.MAXIMAL)) == R.STATUS_MAX


def test_fixture_is_what_its_generator_lists():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_golden_response as M
    finally:
        sys.path.pop(0)
    listed = M.cases()
    assert [{k: v for k, v in c.items() if k != "hex"} for c in GOLDEN["cases"]] == listed


def test_reference_encoder_equals_the_protobuf_runtime():
    pytest.importorskip("google.protobuf")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_golden_response as M
    finally:
        sys.path.pop(0)
    Response = M.message_classes()
    reqs = R.edge_requests() + R.random_requests(11, 400)
    for i, descs in enumerate(reqs):
        keys, gs = R.KEY_SETS[i % len(R.KEY_SETS)], bool(i % 3 == 0)
        code, headers = R.verdict_of(descs, gs)
        want = M.runtime_bytes(Response, code, descs, headers, keys)
        assert R.encode_response(code, descs, headers, keys) == want, i
        m = Response.FromString(want)  # a conforming decoder reads the same answers
        assert m.overall_code == code and len(m.statuses) == len(descs)


# ---- rl_response_serialize, the host twin ----------------------------------------

def host_arrays(reqs, global_shadow):
    """The arrays rl_response_serialize reads: the answers, and the verdict the reference loop gives."""
    req_idx, first, cols = R.arrays_of(reqs)
    res = {k: np.array(v, abi.REQUEST_RESULT_DTYPES[k]) for k, v in cols.items()}
    ver = {k: np.zeros(max(len(reqs), 1), dt) for k, dt in abi.REQUEST_VERDICT_DTYPES.items()}
    for q, descs in enumerate(reqs):
        code, headers = R.verdict_of(descs, global_shadow)
        ver["overall_code"][q] = code
        ver["min_descriptor"][q] = abi.RL_NO_DESCRIPTOR if headers is None else first[q]
        if headers is not None:
            ver["header_limit"][q], ver["header_remaining"][q], ver["header_reset_s"][q] = headers
    return np.array(first, np.uint32), res, ver


def split(raw, off):
    raw = bytes(raw)
    return [raw[int(off[q]):int(off[q + 1])] for q in range(len(off) - 1)]


@pytest.mark.parametrize("keys", R.KEY_SETS, ids=lambda k: "none" if k is None else "keys%d" % len(k[2]))
@pytest.mark.parametrize("global_shadow", [False, True])
def test_host_serializer_equals_the_reference_encoder(keys, global_shadow):
    reqs = R.edge_requests() + R.random_requests(5 + bool(global_shadow), 3000)
    first, res, ver = host_arrays(reqs, global_shadow)
    raw, off = Backend.response_serialize(first, None, res, ver, keys)
    want = [R.encode_request(d, global_shadow, keys) for d in reqs]
    assert off[0] == 0 and int(off[-1]) == len(raw) == sum(map(len, want))
    assert split(raw, off) == want
    assert len(raw) <= Backend.response_bound(len(reqs), int(first[-1]), keys) == R.bound(len(reqs), int(first[-1]), keys)


def test_host_serializer_skips_deferred_and_malformed_requests():
    reqs = R.random_requests(9, 300)
    status = np.zeros(len(reqs), np.uint8)
    for q in range(0, len(reqs), 5):
        reqs[q] = []
        status[q] = 1 + q % 2
    first, res, ver = host_arrays(reqs, False)
    keys = R.KEY_SETS[3]
    raw, off = Backend.response_serialize(first, status, res, ver, keys)
    want = [b"" if status[q] else R.encode_request(d, False, keys) for q, d in enumerate(reqs)]
    assert split(raw, off) == want and b"" in want
    status[next(q for q, d in enumerate(reqs) if d)] = 2  # a request the device refused has no descriptors
    with pytest.raises(RedisError, match="RL_E_INVALID"):
        Backend.response_serialize(first, status, res, ver, keys)


@pytest.mark.parametrize("keys", [None, R.KEY_SETS[2], R.KEY_SETS[4]], ids=["none", "1", "64"])
def test_bound_is_attained_by_the_all_maximal_request(keys):
    for nq, nd in ((1, 1), (3, 7), (40, 2)):
        reqs = [[R.MAXIMAL] * nd for _ in range(nq)]
        first, res, ver = host_arrays(reqs, False)
        # the longest header values: ten digits each
        ver["header_limit"][:] = ver["header_remaining"][:] = ver["header_reset_s"][:] = R.MAX_U32
        raw, off = Backend.response_serialize(first, None, res, ver, keys)
        assert len(raw) == Backend.response_bound(nq, nq * nd, keys) == R.bound(nq, nq * nd, keys)
    assert Backend.response_bound(0, 0, keys) == 0


def test_capacity_answer_reports_the_exact_bytes():
    L = _lib.lib()
    reqs = R.edge_requests()
    first, res, ver = host_arrays(reqs, False)
    keys = R.KEY_SETS[3]
    raw, off = Backend.response_serialize(first, None, res, ver, keys)
    r, v = abi.RlRequestResult(), abi.RlRequestVerdict()
    for k, a in res.items():
        setattr(r, k, abi.ptr(a))
    for k, a in ver.items():
        setattr(v, k, abi.ptr(a))
    f, keep = abi.make_response_format(keys)
    out = np.full(len(raw) + 16, 0x5A, np.uint8)
    off2 = np.zeros(len(reqs) + 1, np.uint32)
    need = C.c_uint64(0)

    def call(cap, buf=out):
        return L.rl_response_serialize(len(reqs), abi.ptr(first), None, C.byref(r), C.byref(v), C.byref(f),
                                       abi.ptr(buf), cap, abi.ptr(off2), C.byref(need))

    assert call(len(raw) - 1) == abi.RL_E_CAPACITY and need.value == len(raw)
    assert (out == 0x5A).all() and off2.tobytes() == off.tobytes()       # nothing written, the offsets known
    assert call(0, None) == abi.RL_E_CAPACITY and need.value == len(raw)
    assert call(len(raw)) == abi.RL_OK and need.value == len(raw)
    assert bytes(out[:len(raw)]) == bytes(raw) and (out[len(raw):] == 0x5A).all()
    # format errors: a key over 64 bytes, a NULL key with a length, a non-zero reserved field
    f65, k65 = abi.make_response_format((b"k" * 65, b"", b""))
    assert L.rl_response_bound(1, 1, C.byref(f65)) == 0
    for bad in ("long", "null", "reserved"):
        g, kg = abi.make_response_format(keys)
        if bad == "long":
            g = f65
        elif bad == "null":
            g.reset_key = None
        else:
            g.reserved = 1
        assert L.rl_response_serialize(len(reqs), abi.ptr(first), None, C.byref(r), C.byref(v), C.byref(g),
                                       abi.ptr(out), len(out), abi.ptr(off2), C.byref(need)) == abi.RL_E_INVALID, bad


# ---- the shared emitter on the CPU, plain and sanitized -------------------------------

@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("resp")
    src = os.path.join(HERE, "c_abi", "resp_emit_run.cpp")
    plain, san = str(d / "resp_emit_run"), str(d / "resp_emit_run_san")
    base = ["g++", "-std=c++17", "-Wall", "-I" + CSRC, src]
    subprocess.run(base + ["-O2", "-o", plain], check=True, capture_output=True, text=True)
    subprocess.run(base + SAN + ["-o", san], check=True, capture_output=True, text=True)
    syms = subprocess.run(["nm", "-u", san], capture_output=True, text=True).stdout
    assert "__asan_report_store" in syms and "__ubsan_handle" in syms  # (instrumented)
    return plain, san, d


def case_file(path, reqs, global_shadow, keys):
    first, res, ver = host_arrays(reqs, global_shadow)
    w = [struct.pack("<I", keys is not None)]
    for k in keys or (b"", b"", b""):
        w.append(struct.pack("<I", len(k)) + k + b"\0" * (-len(k) % 4))
    w.append(struct.pack("<I", len(reqs)))
    for q, descs in enumerate(reqs):
        w.append(struct.pack("<6I", int(ver["overall_code"][q]), int(ver["min_descriptor"][q]),
                             int(ver["header_limit"][q]), int(ver["header_remaining"][q]),
                             int(ver["header_reset_s"][q]), len(descs)))
        for d in descs:
            w.append(struct.pack("<6I", *d))
    with open(path, "wb") as f:
        f.write(b"".join(w))


def _run(exe, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("k", range(len(R.KEY_SETS)))
def test_shared_emitter_equals_the_reference_and_is_clean_under_asan_and_ubsan(drivers, k):
    plain, san, d = drivers
    keys, gs = R.KEY_SETS[k], bool(k % 2)
    reqs = R.edge_requests() + R.random_requests(20 + k, 1500)
    path = str(d / ("cases%d.bin" % k))
    case_file(path, reqs, gs, keys)
    out = _run(plain, path)
    lines = [ln.split(" ") for ln in out.split("\n") if ln.startswith("R ")]
    assert len(lines) == len(reqs)
    for q, (descs, ln) in enumerate(zip(reqs, lines)):
        want = R.encode_request(descs, gs, keys)
        assert (int(ln[1]), int(ln[2]), ln[3]) == (q, len(want), want.hex()), q
    b = [ln.split() for ln in out.split("\n") if ln.startswith("B ")][0]
    assert int(b[1]) == R.bound(len(reqs), sum(map(len, reqs)), keys) >= int(b[2]) == sum(int(ln[2]) for ln in lines)
    assert _run(san, path) == out
