"""Device-interned override rules on the CPU: the ABI additions (header,
exports, the ctypes mirrors against a C99 compiler's layout) and the shared
walk with overrides reported (ratelimit_amd/csrc/rl_wire_parse.h,
walk_message<B, S, false> and descriptor_key) run on the host by
tests/c_abi/wire_override_run.cpp — plain and under AddressSanitizer +
UndefinedBehaviorSanitizer — against the host packer, the authority: which
descriptors carry a limit, the merged requests_per_unit and unit, and the
descriptorKey bytes. No GPU call."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import pytest

from ratelimit_amd import _lib, abi
from ratelimit_amd.config import RequestPacker
import override_cases as OC
import wire_cases as WC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "ratelimit_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
NEW = ("rl_override_rules_enable", "rl_override_rules_info_get", "rl_override_rule_keys")


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(INC, "ratelimit_hip.h")).read()
    assert "#define RL_ABI_VERSION 8u" in text
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    # the header says what the table is not part of
    doc = text[text.index("Override stats keys interned on the GPU"):text.index("typedef struct rl_override_rules_config")]
    for word in ("rl_snapshot_save", "rl_export_range", "rl_resize", "rl_config_load"):
        assert word in doc, word


def test_ctypes_mirrors_equal_the_c99_layout(tmp_path):
    exe = str(tmp_path / "override_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC,
                    os.path.join(HERE, "c_abi", "override_layout.c"), "-o", exe], check=True, capture_output=True,
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
    mirror = {"rl_override_rules_config": abi.RlOverrideRulesConfig, "rl_override_rules_info": abi.RlOverrideRulesInfo}
    assert set(sizes) == set(mirror)
    for name, cls in mirror.items():
        assert C.sizeof(cls) == sizes[name], name
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == fields[name], name
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION}


# ---- the shared walk with overrides reported, on the CPU ---------------------

@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("wire_override")
    src = os.path.join(HERE, "c_abi", "wire_override_run.cpp")
    plain, san = str(d / "wire_override_run"), str(d / "wire_override_run_san")
    base = ["g++", "-std=c++17", "-Wall", "-I" + CSRC, src]
    subprocess.run(base + ["-O2", "-o", plain], check=True, capture_output=True, text=True)
    subprocess.run(base + SAN + ["-o", san], check=True, capture_output=True, text=True)
    syms = subprocess.run(["nm", "-u", san], capture_output=True, text=True).stdout
    assert "__asan_report_load" in syms and "__ubsan_handle" in syms  # (instrumented)
    return plain, san, d


@pytest.fixture(scope="module")
def inputs():
    """(label, message) of every case: the messages, their truncations and byte flips; and what the
    packer says of each one alone."""
    base = OC.messages()
    cases = list(base)
    named = [m for label, m in base if not label.startswith("valid")]
    with_ov = [m for label, m in base if label.startswith("valid") and m][:40]
    cases += [("truncated", m) for m in WC.truncations(named + with_ov[:6])]
    cases += [("flip", m) for m in WC.flips(600, seed=23, msgs=named + with_ov)]
    pk = RequestPacker(first_override_rule=7)
    try:
        want = [OC.packer_overrides(pk, m) for _, m in cases]
        plain = [WC.expect(pk, m)[0] for _, m in cases]
    finally:
        pk.close()
    return cases, want, plain


def _write(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)) + b"".join(struct.pack("<I", len(m)) + m for _, m in cases))


def _run(exe, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def _parse(text):
    """-> per message (status with overrides deferred, status with overrides reported, descriptors, overrides)"""
    out = []
    for ln in text.split("\n"):
        p = ln.split()
        if p and p[0] == "M":
            out.append([int(p[2]), int(p[3]), int(p[4]), int(p[5]), []])
        elif p and p[0] == "D":
            key = b"" if p[5] == "-" else bytes.fromhex(p[5])
            assert len(key) == int(p[4])
            out[-1][4].append((int(p[1]), int(p[2]), int(p[3]), key))
    return out


def test_override_walk_equals_the_host_packer(drivers, inputs):
    plain, _, d = drivers
    cases, want, plain_status = inputs
    path = str(d / "msgs.bin")
    _write(path, cases)
    got = _parse(_run(plain, path))
    assert len(got) == len(cases)
    n_ov = n_bad = n_flip_ov = 0
    by_name = {}
    for (label, m), w, ps, (st0, st1, nd, nov, ovs) in zip(cases, want, plain_status, got):
        # the walk that defers overrides is what it was: the packer's verdict of the message alone
        assert st0 == ps, (label, m[:40])
        if w is None:
            assert st1 == abi.RL_WIRE_MALFORMED and not ovs, (label, m[:40])
            n_bad += 1
            continue
        assert st1 != abi.RL_WIRE_MALFORMED, (label, m[:40])
        assert nd == w[0] and nov == len(w[1]), (label, m[:40])
        assert ovs == w[1], (label, m[:40])
        # an override alone never defers the reporting walk
        if ovs and st1 == abi.RL_WIRE_OK:
            assert st0 == abi.RL_WIRE_DEFERRED
        n_ov += len(ovs)
        n_flip_ov += label == "flip" and bool(ovs)
        if label.startswith("named:"):
            by_name[label[6:]] = ovs
    assert n_ov >= 400 and n_bad >= 300 and n_flip_ov >= 50
    # the named cases, spelled out
    dk = b"domain_1."
    assert by_name["domain_after_descriptors"] == [(0, 10, 1, dk + b"key_x_a_b")]
    assert by_name["domain_twice_around"] == [(0, 10, 1, dk + b"key_x_a_b")]
    assert by_name["no_domain"] == [(0, 10, 1, b".key_x_a_b")]
    assert by_name["two_limits_last_wins"] == [(0, 7, 3, dk + b"k_v")]
    assert by_name["two_limits_merge_fields"] == [(0, 10, 2, dk + b"k_v")]
    assert by_name["limit_fields_repeated"] == [(0, 9, 2, dk + b"k_v")]
    assert by_name["empty_limit"] == [(0, 0, 0, dk + b"k_v")]
    assert by_name["rpu_past_32_bits"] == [(0, 9, 1, dk + b"k_v")]
    assert by_name["empty_value"] == [(0, 3, 1, dk + b"k")]
    assert by_name["alias_a_b_empty"] == by_name["alias_a_b_split"] == [(0, 3, 1, dk + b"a_b")]
    assert by_name["no_entries"] == [(0, 4, 2, dk)]
    assert by_name["key_twice_value_twice"] == [(0, 2, 2, dk + b"key_x_c")]
    assert [o[2] for n in ("unit_0", "unit_absent", "unit_5", "unit_300", "unit_past_32_bits") for o in by_name[n]] == \
        [0, 0, 5, 255, 2]
    assert by_name["four_entries"] == [(0, 8, 4, dk + b"k0_v0.k1_v1.k2_v2.k3_v3")]
    assert [o[0] for o in by_name["override_among_plain"]] == [1, 3]


def test_override_walk_is_clean_under_asan_and_ubsan(drivers, inputs):
    plain, san, d = drivers
    cases, _, _ = inputs
    path = str(d / "msgs_san.bin")
    _write(path, cases)
    assert _run(san, path) == _run(plain, path)


def test_sinks_without_the_member_compile_and_the_existing_driver_builds(tmp_path):
    """tests/c_abi/wire_parse_run.cpp (its sinks have no limit() member) builds unmodified against the header."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "wire_parse_run")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(HERE, "c_abi", "wire_parse_run.cpp"),
                    "-O2", "-o", exe], check=True, capture_output=True, text=True)
    path = str(tmp_path / "one.bin")
    _write(path, [("override", dict(WC.extra_cases())["override"]), ("plain", dict(WC.extra_cases())["two_byte_length"])])
    lines = [ln.split() for ln in _run(exe, path).split("\n") if ln.startswith("M ")]
    assert [int(ln[2]) for ln in lines] == [abi.RL_WIRE_DEFERRED, abi.RL_WIRE_OK]
