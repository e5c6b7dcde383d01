"""CPU-side checks of the per-request verdict (rl_do_limit_requests_verdict /
rl_debug_verdict): the header declares both and the library exports them under
ABI 8; the ctypes mirror of rl_request_verdict equals the C compiler's layout
of include/ratelimit_hip.h; the sequential restatement of ratelimit.go:163-209
(tests/verdict_ref.py) reproduces the reference's own service tests
(tests/golden/ref_service_verdict.json)."""
import ctypes as C
import json
import os
import subprocess

import pytest

import verdict_ref as V
from ratelimit_amd import abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "ratelimit_hip.h")
LIB = os.path.join(ROOT, "ratelimit_amd", "libratelimit_hip.so")
CFLAGS = ["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC]
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_service_verdict.json")))

NEW = ("rl_do_limit_requests_verdict", "rl_debug_verdict")


def test_header_declares_and_library_exports_the_verdict_calls():
    src = " ".join(open(HEADER).read().split())
    assert ("int rl_do_limit_requests_verdict(rl_ctx* ctx, const rl_request_batch* in, rl_request_result* out, "
            "uint32_t opts, rl_request_verdict* verdict);") in src
    assert "int rl_debug_verdict(rl_ctx* ctx, uint32_t n_requests, uint32_t n_descriptors," in src
    assert "#define RL_ABI_VERSION 8u" in src  # additive: the version stays
    if not os.path.exists(LIB):
        from ratelimit_amd import build
        build.build()
    lib = C.CDLL(LIB)
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    lib.rl_abi_version.restype = C.c_uint32
    assert lib.rl_abi_version() == abi.ABI_VERSION == 8


def test_verdict_struct_matches_the_c_layout(tmp_path):
    exe = str(tmp_path / "verdict_layout")
    subprocess.run(CFLAGS + [os.path.join(ROOT, "tests", "c_abi", "verdict_layout.c"), "-o", exe], check=True,
                   capture_output=True, text=True)
    sizes, fields, consts = {}, [], {}
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] == "S":
            sizes[p[1]] = int(p[2])
        elif p[0] == "F":
            assert p[1] == "rl_request_verdict"
            fields.append((p[2], int(p[3]), int(p[4])))
        else:
            consts[p[1]] = int(p[2])
    cls = abi.RlRequestVerdict
    assert sizes == {"rl_request_verdict": C.sizeof(cls)}
    assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == fields
    assert consts == {"RL_ABI_VERSION": abi.ABI_VERSION, "RL_NO_DESCRIPTOR": abi.RL_NO_DESCRIPTOR,
                      "RL_VERDICT_OVER_LIMIT": abi.RL_VERDICT_OVER_LIMIT,
                      "RL_VERDICT_GLOBAL_SHADOW": abi.RL_VERDICT_GLOBAL_SHADOW,
                      "RL_VERDICT_OPT_GLOBAL_SHADOW": abi.RL_VERDICT_OPT_GLOBAL_SHADOW}
    # the per-request arrays the Python side allocates are the struct's pointer fields, global_shadow apart
    assert list(abi.REQUEST_VERDICT_DTYPES) + ["global_shadow"] == [f for f, _ in cls._fields_]
    assert (V.FLAG_OVER_LIMIT, V.FLAG_GLOBAL_SHADOW) == (abi.RL_VERDICT_OVER_LIMIT, abi.RL_VERDICT_GLOBAL_SHADOW)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["source"])
def test_restatement_reproduces_the_reference_service_tests(case):
    got = V.verdict(V.golden_statuses(case), case["is_unlimited"], case["global_shadow_mode"])
    exp = case["expect"]
    assert got.code == exp["overall_code"]
    assert got.shadow_inc == exp["global_shadow_mode_counter"]
    if case["headers_enabled"]:  # ResponseHeadersToAdd: strconv.FormatUint of the three values
        assert [str(x) for x in got.headers] == exp["headers"]
        assert exp["headers"] == ["10", "0", "58"]


def test_restatement_edges():
    """The loop's order dependence, on vectors small enough to follow by hand."""
    L = V.Limit(10, 2)

    def s(code, rem, limited=True):
        return V.Status(code, L if limited else None, rem, 58 if limited else None)

    # the last OVER_LIMIT wins, whatever comes between or after with remaining 0
    v = V.verdict([s(2, 0), s(1, 0), s(2, 0), s(1, 0)], [False] * 4, False)
    assert (v.code, v.min_index) == (2, 2)
    # no OVER_LIMIT: the first of the smallest remaining (strict <)
    v = V.verdict([s(1, 5), s(1, 3), s(1, 3), s(1, 7)], [False] * 4, False)
    assert (v.code, v.min_index, v.headers) == (1, 1, (10, 3, 58))
    # unlimited and unmatched descriptors carry no CurrentLimit: never chosen
    v = V.verdict([s(1, V.MAX_U32, False), s(1, 0, False)], [True, False], True)
    assert v == V.Verdict(1, 0, None, None, 0)
    # a limited descriptor with MaxUint32 remaining is not below the starting minimum
    v = V.verdict([s(1, V.MAX_U32)], [False], False)
    assert v.min_index is None
    # global shadow mode keeps the headers and counts once per request
    v = V.verdict([s(2, 0), s(2, 0)], [False, False], True)
    assert v == V.Verdict(1, 3, 1, (10, 0, 58), 1)
    assert V.verdict([], [], True) == V.Verdict(1, 0, None, None, 0)
