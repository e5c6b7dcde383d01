"""The maintenance calls' pure host logic (no GPU): rl_stem_list.h, the one check
of a CSR stem list, and rl_shard_split.h, the split of a stem list by owning
shard, compiled for the host with g++ (plain, and under AddressSanitizer +
UndefinedBehaviorSanitizer) into a stand-alone program
(tests/c_abi/maint_host_run.cpp) whose answers are compared with the same
logic restated here."""
import os
import shutil
import subprocess

import pytest

from ratelimit_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
NONE, START, ENTRY, TOTAL = 0, 1, 2, 3
ANY = 0xFFFFFFFF


def stem_expect(allow_empty, max_len, cap, off):
    """The engine's checks as they were written out per call: the first offset,
    then entry by entry, then the total. -> (fault, entry)."""
    n = len(off) - 1
    if n == 0:
        return NONE, 0
    if off[0] != 0:
        return START, 0
    for i in range(n):
        a, b = off[i], off[i + 1]
        if b < a or (b == a and not allow_empty) or b - a > max_len:
            return ENTRY, i
    return (TOTAL if off[n] > cap else NONE), 0


def stem_cases():
    out = []
    # (rl_forget's rule; rl_lookup's; rl_scan's)
    for allow_empty, max_len in ((0, 65535), (1, ANY), (0, ANY)):
        def case(off, cap=1 << 20):
            out.append((allow_empty, max_len, cap, list(off)))
        case([0])                                   # n = 0 (the offsets are not looked at)
        case([7])
        case([0, 5])                                # one entry
        case([1, 5])                                # off[0] != 0
        case([3, 3])
        case([0, 4, 8, 6, 12])                      # an offset that decreases
        case([0, 4, 4, 8])                          # an empty entry: allowed or not
        case([0, 0])
        case([0, 65535])                            # the longest entry, and one byte more
        case([0, 65536])
        case([0, 4, 65539, 65543])
        case([0, 4, 65540, 65544])
        case([0, 100, 200], cap=200)                # a total exactly at the cap, and one over it
        case([0, 100, 201], cap=200)
        case([0, 100, 201], cap=0)
        for bad in (0, 2, 4):                       # the entry reported: first, middle, last
            off = [0, 4, 8, 12, 16, 20]
            for k in range(bad + 1, 6):
                off[k] -= 4                         # entry `bad` is empty
            case(off)
            off = [0, 4, 8, 12, 16, 20]
            off[bad + 1] = off[bad] + 70000         # entry `bad` is too long (the next one then decreases)
            case(off)
        case([0, 1, 0])                             # decreasing at the last entry
        case([0, ANY])                              # (no 32-bit wrap in the length)
        case([0] + [4 * k for k in range(1, 1200)] + [3], cap=1 << 30)  # a long list, its last entry decreasing
    return out


def fnv1a(b):
    h = 2166136261
    for x in b:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h


def split_expect(n_shards, one, lens):
    part = [([], [0], bytearray()) for _ in range(n_shards)]
    for i, ln in enumerate(lens):
        stem = bytes((i * 7 + k) & 255 for k in range(ln))
        idx, off, blob = part[n_shards - 1 if one else fnv1a(stem) % n_shards]
        idx.append(i)
        blob += stem
        off.append(len(blob))
    for idx, off, blob in part:  # the sub-lists' offsets start at 0 and end at the bytes gathered
        assert off[0] == 0 and off[-1] == len(blob) and len(off) == len(idx) + 1
    return " | ".join("%s;%s;%s" % (",".join(map(str, idx)), ",".join(map(str, off)), blob.hex())
                      for idx, off, blob in part) + " # ok"


def split_cases():
    out = []
    for n in (0, 1, 37):
        for shards in (1, 2, 3, 16):
            for one in (0, 1):
                out.append((shards, one, [(5 * i + 3) % 23 + 1 for i in range(n)]))
                out.append((shards, one, [0] * n))                      # all-empty stems
                out.append((shards, one, [(i % 3) * 40 for i in range(n)]))  # some empty, some long
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """-> {build: the program's answer lines}, each build compiled and run once."""
    assert shutil.which("g++"), "the host build of rl_stem_list.h / rl_shard_split.h needs g++"
    lines = ["stem %d %d %d %d %s" % (e, m, c, len(off) - 1, " ".join(map(str, off)))
             for e, m, c, off in stem_cases()]
    lines += ["split %d %d %d %s" % (s, o, len(lens), " ".join(map(str, lens))) for s, o, lens in split_cases()]
    got = {}
    for name, flags in (("plain", ["-O2"]), ("asan_ubsan", SAN)):
        exe = str(tmp_path_factory.mktemp(name) / "maint_host_run")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "ratelimit_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c_abi", "maint_host_run.cpp"), "-o", exe] + flags, check=True,
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
def test_stem_list_check_on_the_host(answers, which):
    """n = 0; one entry; off[0] != 0; a decreasing offset; an empty entry where
    allowed and where not; 65535 bytes accepted and 65536 refused; a total at
    the cap and over it; the entry reported for a failure at the first, a
    middle and the last entry: fault and entry, under each call's rule. (The
    words around them are pinned on the GPU: tests/test_gpu_maint_errors.py.)"""
    cases = stem_cases()
    assert len(cases) >= 3 * 24
    seen = set()
    for (e, m, c, off), line in zip(cases, answers[which]):
        fault, entry = stem_expect(e, m, c, off)
        assert line == "%d %d" % (fault, entry), (e, m, c, off[:8])
        seen.add(((e, m), fault))
    assert seen == {(r, f) for r in ((0, 65535), (1, ANY), (0, ANY)) for f in (NONE, START, ENTRY, TOTAL)}
    assert stem_expect(0, 65535, 1 << 20, [0, 65535]) == (NONE, 0)
    assert stem_expect(0, 65535, 1 << 20, [0, 65536]) == (ENTRY, 0)
    assert stem_expect(1, ANY, 200, [0, 100, 201]) == (TOTAL, 0)
    assert stem_expect(0, ANY, 4096, [0, 4, 4]) == (ENTRY, 1)


@pytest.mark.parametrize("which", ["plain", "asan_ubsan"])
def test_shard_split_on_the_host(answers, which):
    """0, 1 and 37 records over 1, 2, 3 and 16 shards, by a hash and all to one
    shard (the others empty), all-empty stems: each shard's indices in the
    caller's order, its sub-list's offsets from 0 to the bytes gathered, its
    bytes; put(take(x)) == x for a u8, a u32 and an i64 column."""
    cases = split_cases()
    lines = answers[which][len(stem_cases()):]
    assert len(lines) == len(cases) == 3 * 4 * 2 * 3
    for (shards, one, lens), line in zip(cases, lines):
        assert line == split_expect(shards, one, lens), (shards, one, len(lens))
    # the 37 records over 16 shards by hash do spread, and the one-shard functor leaves the rest empty
    spread = split_expect(16, 0, [(5 * i + 3) % 23 + 1 for i in range(37)]).split(" # ")[0].split(" | ")
    assert sum(1 for p in spread if not p.startswith(";")) >= 8
    lone = split_expect(16, 1, [4] * 37).split(" # ")[0].split(" | ")
    assert all(p == ";0;" for p in lone[:-1]) and lone[-1].startswith("0,1,2,")


def test_the_new_files_are_built():
    assert "rl_maint.hip" in build.SOURCES and build.SOURCES[0] == "rl_kernels.hip"
    for h in ("rl_stem_list.h", "rl_shard_split.h", "rl_engine_int.h"):
        assert h in build.HEADERS
