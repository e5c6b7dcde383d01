"""The request path's pure host arithmetic (no GPU): rl_request_layout.h (the
carve of a device buffer, match_pieces, in_buf, index_ends_ok, tiles) compiled
for the host with g++ (plain, and under AddressSanitizer +
UndefinedBehaviorSanitizer) into a stand-alone program
(tests/c_abi/request_layout_run.cpp), its answers compared with the formula the
calls wrote out one by one before rl_requests.hip: over a buffer's pieces, the
sum of max(bytes, 1) rounded up to 256."""
import glob
import itertools
import os
import re
import shutil
import subprocess

import pytest

from ratelimit_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ratelimit_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
NS, NQS, NES = (0, 1, 3, 64), (0, 1, 255, 256, 257), (0, 1, 7)
M64 = (1 << 64) - 1


def verdict_bytes(nq):
    """verdict_layout(nq).bytes (rl_match.h)."""
    return ((12 * nq + 7) & ~7) + 8 + 16 * nq + 2 * nq


def scan_bytes(n):
    """A stand-in for match_scan_bytes(n): a number of its own per n, no multiple of 256."""
    return 1000 + 8 * n if n else 0


def carve(pieces):
    """The formula of the calls before the layer -> (total, {name: offset})."""
    need, offs = 0, {}
    for name, nbytes in pieces:
        offs[name] = need
        need += (max(nbytes, 1) + 255) & ~255
    return need, offs


def match_list(n, scan, verdict, nq):
    out = [("v", n * 16), ("kind", n * 4), ("rpu", n * 4), ("rule", n * 4), ("cnt", 16), ("code", n), ("rem", n * 4),
           ("reset", n * 4), ("match", n), ("orule", n * 4), ("orpu", n * 4), ("ounit", n), ("tmp", scan)]
    return out + ([("verdict", verdict_bytes(nq))] if verdict else [])


def layout_cases():
    """-> [(query line, the buffer's pieces)], in the order the calls carved them before the layer, except the
    wire middle stage's: there the verdict block came after the override arrays and now comes before them (the
    total, a sum, is the same)."""
    out = []
    for n, nq, ne in itertools.product(NS, NQS, NES):
        dom, desc, scan, vb = 3 * nq, 11 * ne, scan_bytes(n), verdict_bytes(nq)
        for ovr, verdict in itertools.product((0, 1), (0, 1)):
            o = n if ovr else 0
            out.append(("sync %d %d %d %d %d %d %d %d %d" % (n, nq, ne, dom, desc, ovr, scan, verdict, vb),
                        [("dom", dom), ("domoff", (nq + 1) * 4), ("hits", nq * 4), ("req", n * 4), ("ent", (n + 1) * 4),
                         ("doff", (n + 1) * 4), ("desc", desc), ("kl", ne * 2), ("vl", ne * 2), ("ovf", o),
                         ("ovr", o * 4), ("ovu", o), ("ovrule", o * 4)] + match_list(n, scan, verdict, nq)))
            if ne == 0:  # (the packed mbuf does not depend on the entries)
                out.append(("packed %d %d %d %d %d %d" % (n, nq, ovr, scan, verdict, vb),
                            [("domoff", (nq + 1) * 4), ("req", n * 4), ("ent", (n + 1) * 4), ("doff", (n + 1) * 4),
                             ("ov", n * 10 if ovr else 0)] + match_list(n, scan, verdict, nq)))
            for resp in (0, 1):
                rb = 777 + 5 * nq + n
                out.append(("wiremid %d %d %d %d %d %d %d %d %d %d %d" % (n, nq, ne, dom, desc, ovr, scan, verdict, vb,
                                                                           resp, rb),
                            [("domoff", (nq + 1) * 4), ("req", n * 4), ("ent", (n + 1) * 4), ("doff", (n + 1) * 4),
                             ("hits", nq * 4), ("klen", ne * 2), ("vlen", ne * 2), ("dom", dom), ("desc", desc)] +
                            match_list(n, scan, verdict, nq) + ([("ov", n * 10)] if ovr else []) +
                            ([("resp", rb)] if resp else [])))
    for nq in NQS:
        T = (nq + 255) // 256
        for ovr in (0, 1):
            out.append(("wbuf %d %d %d" % (nq, T, ovr),
                        [("reqw", nq * 16), ("tsum", T * 16), ("index", (T + 1) * 16), ("cnt", 32), ("status", nq),
                         ("first", (nq + 1) * 4)] + ([("miss", nq * 4)] if ovr else [])))
    return out


def in_buf_cases():
    B = 4096
    return [(B, B, 0), (B, B, 1), (B, B + 4, 0), (B, 100, B - 100), (B, 100, B - 100 + 1), (B, 0, B), (B, 0, B + 1),
            (B, 101, 4), (B, 102, 4), (B, 103, 0), (B, 8, M64 - 7), (B, 8, M64), (B, M64 - 3, 8), (M64, M64 - 3, 3),
            (0, 0, 0), (0, 0, 1), (0, 4, 0)]


def ends_cases():
    out = []
    for T in (0, 1, 2):
        base = [0, 0, 0, 0] + [9] * (4 * (T - 1) if T else 0) + ([5, 7, 11, 13] if T else [])
        base = base[:4 * (T + 1)] if T else [0, 0, 0, 0]
        n, ne = (5, 7) if T else (0, 0)
        out += [(T, n, None, list(base)), (T, n, ne, list(base)), (T, n + 1, None, list(base)),
                (T, n, ne + 1, list(base))]
        for w in range(4):  # a first entry that is not zero (with T == 0 it is also the last)
            bad = list(base)
            bad[w] += 1
            out.append((T, bad[0] if T == 0 else n, None, bad))
    return out


def ends_expect(T, n, ne, ix):
    return int(not any(ix[:4]) and ix[4 * T] == n and (ne is None or ix[4 * T + 1] == ne))


TILE_CASES = [(nq, 256) for nq in (0, 1, 255, 256, 257, 513)] + [(0, 1), (5, 1)]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """-> {build: the program's answer lines}, each build compiled and run once."""
    assert shutil.which("g++"), "the host build of rl_request_layout.h needs g++"
    lines = [q for q, _ in layout_cases()] + ["in_buf %d %d %d" % c for c in in_buf_cases()]
    lines += ["ends %d %d %s %s" % (T, n, "-" if ne is None else ne, " ".join(map(str, ix))) for T, n, ne, ix in ends_cases()]
    lines += ["tiles %d %d" % c for c in TILE_CASES]
    got = {}
    for name, flags in (("plain", ["-O2"]), ("asan_ubsan", SAN)):
        exe = str(tmp_path_factory.mktemp(name) / "request_layout_run")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                        os.path.join(ROOT, "tests", "c_abi", "request_layout_run.cpp"), "-o", exe] + flags, check=True,
                       capture_output=True, text=True)
        if flags is SAN:
            syms = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
            assert "__asan_" in syms and "__ubsan_handle" in syms  # (instrumented)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        got[name] = r.stdout.split("\n")[:-1]
        assert len(got[name]) == len(lines)
    return got


@pytest.mark.parametrize("which", ["plain", "asan_ubsan"])
def test_buffers_are_carved_as_before_the_layer(answers, which):
    """The sync buffer, mbuf (packed and wire middle) and wbuf over n in {0, 1, 3, 64}, nq in {0, 1, 255, 256, 257},
    ne in {0, 1, 7}, with and without overrides, verdict and respond: the total equals the old formula's byte for
    byte, every piece is 256-aligned, the pieces are disjoint and hold their bytes, and a piece of no bytes still has
    an address of its own."""
    cases = layout_cases()
    assert len(cases) > 700
    kinds = set()
    for (query, pieces), line in zip(cases, answers[which]):
        total, want = carve(pieces)
        words = line.split()
        got = {k: int(v) for k, v in (w.split("=") for w in words[1:])}
        assert int(words[0]) == total, query
        assert set(got) == set(want), query
        spans = sorted((got[name], max(nbytes, 1)) for name, nbytes in pieces)
        assert all(o % 256 == 0 for o, _ in spans), query
        assert len({o for o, _ in spans}) == len(spans), query       # (a zero-byte piece is still distinct)
        for (o, b), (o2, _) in zip(spans, spans[1:] + [(total, 0)]):
            assert o + b <= o2, query                                # disjoint, and inside the total
        kinds.add(query.split()[0])
    assert kinds == {"sync", "packed", "wiremid", "wbuf"}


@pytest.mark.parametrize("which", ["plain", "asan_ubsan"])
def test_section_index_and_tile_checks(answers, which):
    """in_buf at off == B, at bytes == B - off and one more, at an odd offset and with off + bytes wrapping 64 bits;
    index_ends_ok over 0, 1 and 2 tiles; tiles at 0, 255, 256, 257."""
    lines = answers[which][len(layout_cases()):]
    ib, en = in_buf_cases(), ends_cases()
    for (B, off, nbytes), line in zip(ib, lines):
        assert int(line) == int(off % 4 == 0 and off <= B and nbytes <= B - off), (B, off, nbytes)
    assert [int(x) for x in lines[:7]] == [1, 0, 0, 1, 0, 1, 0]
    assert [int(x) for x in lines[10:13]] == [0, 0, 0]               # off + bytes wraps: refused all the same
    for (T, n, ne, ix), line in zip(en, lines[len(ib):]):
        assert int(line) == ends_expect(T, n, ne, ix), (T, n, ne, ix)
    assert {ends_expect(*c) for c in en} == {0, 1}
    for (nq, tile), line in zip(TILE_CASES, lines[len(ib) + len(en):]):
        assert int(line) == (nq + tile - 1) // tile
    assert [(nq + 255) // 256 for nq in (0, 255, 256, 257)] == [0, 1, 1, 2]


def test_the_layer_is_built_and_the_copies_are_gone():
    assert "rl_requests.hip" in build.SOURCES and "rl_request_layout.h" in build.HEADERS
    assert build.SOURCES.index("rl_requests.hip") == build.SOURCES.index("rl_engine.hip") + 1
    # (resp_layout's own carve stays: rl_resp.hip is one of the kernel sources the layer leaves unedited)
    for path in glob.glob(os.path.join(CSRC, "*")):
        text = open(path).read()
        assert os.path.basename(path) == "rl_resp.hip" or "auto piece = [" not in text, path
        assert "auto sect = [" not in text, path
    req = open(os.path.join(CSRC, "rl_requests.hip")).read()
    eng = open(os.path.join(CSRC, "rl_engine.hip")).read()
    for one in (r"\nReqDev req_dev\(", r"\nRefusal match_fail\(", r"\nint slot_submit_begin\(", r"\nvoid slot_pend\("):
        assert len(re.findall(one, req)) == 1 and not re.search(one, eng), one
    for one in (r"\nint grow\(", r"\nrl_batch staged_batch\("):
        assert len(re.findall(one, eng)) == 1 and not re.search(one, req), one
    # (one growth sequence: nothing else frees and re-allocates a buffer by its cap)
    assert len(re.findall(r"_cap = 0;", req + eng)) == 0 and (req + eng).count("*cap = 0;") == 1
