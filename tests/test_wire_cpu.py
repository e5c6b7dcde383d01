"""rl_do_limit_wire_async on the CPU: the ABI additions (header, exports, the
ctypes mirrors against a C99 compiler's layout), Backend.wire_batch's buffer
against a pure-Python decode, and the per-message walk the kernels share
(ratelimit_amd/csrc/rl_wire_parse.h) run on the host by
tests/c_abi/wire_parse_run.cpp — plain and under AddressSanitizer +
UndefinedBehaviorSanitizer — against the host packer, the authority: packer
error -> MALFORMED, override or per-item limit -> DEFERRED, otherwise OK with
the packer's arrays. No GPU call."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from ratelimit_amd import _lib, abi
from ratelimit_amd.config import RequestPacker
from ratelimit_amd.limiter import Backend
import wire_cases as WC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "ratelimit_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(INC, "ratelimit_hip.h")).read()
    assert re.search(r"\bint\s+rl_do_limit_wire_async\s*\(", text)
    assert "#define RL_ABI_VERSION 8u" in text
    assert "rl_do_limit_wire_async" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "rl_do_limit_wire_async") and L.rl_abi_version() == 8


def test_ctypes_mirrors_equal_the_c99_layout(tmp_path):
    exe = str(tmp_path / "wire_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC,
                    os.path.join(HERE, "c_abi", "wire_layout.c"), "-o", exe], check=True, capture_output=True, text=True)
    sizes, fields, consts = {}, {}, {}
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n"):
        p = ln.split()
        if p and p[0] == "S":
            sizes[p[1]] = int(p[2])
        elif p and p[0] == "F":
            fields.setdefault(p[1], []).append((p[2], int(p[3]), int(p[4])))
        elif p and p[0] == "C":
            consts[p[1]] = int(p[2])
    mirror = {"rl_wire_batch": abi.RlWireBatch, "rl_wire_result": abi.RlWireResult}
    assert set(sizes) == set(mirror)
    for name, cls in mirror.items():
        assert C.sizeof(cls) == sizes[name], name
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == fields[name], name
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION, "RL_WIRE_TILE": abi.RL_WIRE_TILE,
                      "RL_REQUESTS_TILE": abi.RL_REQUESTS_TILE, "RL_WIRE_OK": abi.RL_WIRE_OK,
                      "RL_WIRE_DEFERRED": abi.RL_WIRE_DEFERRED, "RL_WIRE_MALFORMED": abi.RL_WIRE_MALFORMED}
    assert abi.RL_WIRE_TILE == 256 and abi.RL_WIRE_TILE == abi.RL_REQUESTS_TILE
    assert (abi.RL_WIRE_OK, abi.RL_WIRE_DEFERRED, abi.RL_WIRE_MALFORMED) == (0, 1, 2)


def _decode(wb):
    """rl_wire_batch by the header's words alone: [(message bytes, now)]."""
    s, raw = wb.struct, bytes(wb.buf[:wb.struct.buf_bytes])
    nq = s.n_requests
    off = struct.unpack_from("<%dI" % (nq + 1), raw, s.msg_off)
    now = struct.unpack_from("<%dI" % nq, raw, s.now)
    assert off[0] == 0 and off[nq] == s.msgs_bytes
    return [(raw[s.msgs + off[q]:s.msgs + off[q + 1]], now[q]) for q in range(nq)]


@pytest.mark.parametrize("nq", [0, 1, 255, 256, 257, 513])
def test_wire_batch_layout(nq):
    msgs = WC.valid_messages(5, max(nq, 1))[:nq]
    for q in range(0, nq, 7):
        msgs[q] = b""  # empty messages, the first one among them
    nows = [1_700_000_000 + q for q in range(nq)]
    wb = Backend.wire_batch(msgs, nows, None, 3)
    s = wb.struct
    assert (s.n_requests, s.n_rules, wb.n_requests) == (nq, 3, nq)
    assert s.msgs_bytes == sum(len(m) for m in msgs) == wb.msgs_bytes
    for o in (s.msg_off, s.now, s.msgs, s.buf_bytes):
        assert o % 4 == 0
    # the sections lie inside buf and do not overlap
    sect = sorted([(s.msg_off, 4 * (nq + 1)), (s.now, 4 * nq), (s.msgs, s.msgs_bytes)])
    end = 0
    for o, b in sect:
        assert o >= end
        end = o + b
    assert end <= s.buf_bytes <= len(wb.buf) and s.buf == wb.buf.ctypes.data
    assert _decode(wb) == list(zip(msgs, nows))


def test_wire_batch_of_only_empty_messages():
    wb = Backend.wire_batch([b""] * 300, [7] * 300)
    assert wb.struct.msgs_bytes == 0 and _decode(wb) == [(b"", 7)] * 300


# ---- the shared walk on the CPU ---------------------------------------------

@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("wire")
    src = os.path.join(HERE, "c_abi", "wire_parse_run.cpp")
    plain, san = str(d / "wire_parse_run"), str(d / "wire_parse_run_san")
    base = ["g++", "-std=c++17", "-Wall", "-I" + CSRC, src]
    subprocess.run(base + ["-O2", "-o", plain], check=True, capture_output=True, text=True)
    subprocess.run(base + SAN + ["-o", san], check=True, capture_output=True, text=True)
    syms = subprocess.run(["nm", "-u", san], capture_output=True, text=True).stdout
    assert "__asan_report_load" in syms and "__ubsan_handle" in syms  # (instrumented)
    return plain, san, d


@pytest.fixture(scope="module")
def inputs():
    """(label, message) of every case, and each one's expectation from the packer."""
    valid = WC.valid_messages()
    cases = [("sanitize", m) for m in WC.sanitize_messages()]
    cases += [("truncated", m) for m in WC.truncations(valid[:3])]
    cases += [("flip", m) for m in WC.flips(300)]
    cases += [("malformed", m) for m in WC.malformed()]
    cases += [("extra:" + name, m) for name, m in WC.extra_cases()]
    pk = RequestPacker(first_override_rule=7)
    try:
        want = [WC.expect(pk, m) for _, m in cases]
    finally:
        pk.close()
    return cases, want


def _run(exe, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_parse_header_equals_the_host_packer(drivers, inputs):
    plain, _, d = drivers
    cases, want = inputs
    path = str(d / "msgs.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)) + b"".join(struct.pack("<I", len(m)) + m for _, m in cases))
    lines = [ln.split() for ln in _run(plain, path).split("\n") if ln.startswith("M ")]
    assert len(lines) == len(cases)
    seen = {abi.RL_WIRE_OK: 0, abi.RL_WIRE_DEFERRED: 0, abi.RL_WIRE_MALFORMED: 0}
    flip_bad = flip_ok = 0
    for (label, m), (status, arrays), ln in zip(cases, want, lines):
        assert int(ln[2]) == status, (label, m[:40], ln)
        seen[status] += 1
        if status == abi.RL_WIRE_OK:
            assert ln[3] == "%016x" % WC.arrays_fnv(arrays), (label, m[:40])
        else:
            assert ln[3] == "0" * 16
        if label == "flip":
            flip_bad += status == abi.RL_WIRE_MALFORMED
            flip_ok += status != abi.RL_WIRE_MALFORMED
    assert flip_bad >= 50 and flip_ok >= 50  # (the flips exercise both verdicts)
    assert min(seen.values()) >= 50
    # the named cases land where rl_do_limit_wire_async's contract puts them
    by_name = {label[6:]: st for (label, _), (st, _) in zip(cases, want) if label.startswith("extra:")}
    for name in ("override", "override_empty", "descriptors_65536", "entries_65536", "domain_65536"):
        assert by_name[name] == abi.RL_WIRE_DEFERRED, name
    for name in ("key_65536", "override_malformed"):
        assert by_name[name] == abi.RL_WIRE_MALFORMED, name
    for name in ("descriptors_65535", "value_65535", "descriptors_300", "entries_70", "key_300_value_5000",
                 "overlong_varint_length", "hits_past_32_bits", "domain_as_varint", "empty"):
        assert by_name[name] == abi.RL_WIRE_OK, name


def test_parse_header_is_clean_under_asan_and_ubsan(drivers, inputs):
    plain, san, d = drivers
    cases, _ = inputs
    path = str(d / "msgs_san.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)) + b"".join(struct.pack("<I", len(m)) + m for _, m in cases))
    assert _run(san, path) == _run(plain, path)
