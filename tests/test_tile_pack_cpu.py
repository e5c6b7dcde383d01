"""The tile record's pack / unpack helper (ratelimit_amd/csrc/rl_tile.h) on the
host: tests/c_abi/tile_pack_run.cpp built once plain and once under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.
Index 0 and 2^23 - 1, hits 0, 510, 511 and 2^32 - 1 (and the values around
them) each round-trip or flag the escape; an escaped record reads the hits
array at its own index only (the array ends right after it, so ASan sees any
other read)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "c_abi", "tile_pack_run.cpp")
INC = "-I" + os.path.join(ROOT, "ratelimit_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_tile_record_round_trips_or_flags_the_escape(tmp_path, flags):
    assert shutil.which("g++"), "the host build of rl_tile.h needs g++"
    exe = str(tmp_path / "tile_pack_run")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", INC, SRC, "-o", exe] + flags, check=True,
                   capture_output=True, text=True)
    if flags is SAN:
        syms = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
        assert "__asan_" in syms and "__ubsan_handle" in syms  # (instrumented)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) == 11 * 16 * 6
