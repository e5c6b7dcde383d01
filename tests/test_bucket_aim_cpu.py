"""tests/bucket_aim.py without a GPU: the restated stem hash against the
library's host reference, the compositions of test_gpu_big_bucket_paths.py
against the route the model predicts for them, the stem finder, the constants
the model restates against the kernels' source text, and the model's own
power (a mutated composition changes its route)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bucket_aim as A
from ratelimit_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ratelimit_amd", "csrc")
HIP_INC = os.path.join(os.path.dirname(os.path.dirname(build.HIPCC)), "include")
SEEDS = (1, 7, A.SEED, 0xFFFFFFFFFFFFFFFF)


def _stems():
    """(seed, stem): every length 1 .. 40 (tails of 1 .. 7 bytes and the empty
    tail at 8, 16, 24, 32, 40) with random bytes under several seeds, bytes
    0x00 / 0xFF, and aim stems."""
    rng = np.random.default_rng(5)
    out = []
    for seed in SEEDS:
        for n in range(1, 41):
            out.append((seed, rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
            out.append((seed, bytes([0xFF]) * n if n & 1 else bytes(n)))
        out += [(seed, bytes(s)) for s in A.aim_stems([0, 1, 9_999_999_999, 8388607])]
    return out


def test_numpy_hash_equals_the_scalar_restatement():
    by = {}
    for seed, s in _stems():
        by.setdefault((seed, len(s)), []).append(s)
    n = 0
    for (seed, L), group in by.items():
        key = A.hash_key(seed)
        got = A.stem_hash_np(key, np.frombuffer(b"".join(group), np.uint8).reshape(len(group), L))
        assert [int(x) for x in got] == [A.stem_hash(key, s) for s in group], (seed, L)
        n += len(group)
    assert n >= 300
    ids = np.arange(1000, 1400)
    assert [int(x) for x in A.sort_keys(A.SEED, ids)] == [
        A.stem_hash(A.hash_key(A.SEED), b"aim_%010d_x" % i) >> 32 for i in ids]


def test_numpy_hash_equals_hash_stem_host(tmp_path):
    """rl_device.h compiled for the host (tests/c_abi/stem_hash_run.cpp)."""
    assert shutil.which("g++"), "the host build of rl_device.h needs g++"
    exe = str(tmp_path / "stem_hash_run")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + CSRC,
                    "-isystem", HIP_INC, os.path.join(ROOT, "tests", "c_abi", "stem_hash_run.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    cases = _stems()
    text = "".join("%d %s\n" % (seed, s.hex()) for seed, s in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    host = [int(x, 16) for x in r.stdout.split()]
    assert len(host) == len(cases) >= 300
    for (seed, s), h in zip(cases, host):
        assert A.stem_hash(A.hash_key(seed), s) == h, (seed, s)
        assert int(A.stem_hash_np(A.hash_key(seed), np.frombuffer(s, np.uint8)[None, :])[0]) == h, (seed, s)


@pytest.mark.parametrize("name", sorted(A.COMPOSITIONS))
def test_model_predicts_the_route_each_composition_is_aimed_at(name):
    a = A.aimed(name)
    assert a.n <= 12 * 1024 and len(a.buckets) == len(A.COMPOSITIONS[name])
    stems = A.aim_stems(a.ids)
    bucket_of = (A.stem_hash_np(A.hash_key(a.seed), stems) >> np.uint64(54)).astype(np.int64)
    for b, r in zip(a.buckets, a.routes()):
        sp, keys = b["spec"], b["keys"]
        assert r["route"] == sp["route"], r
        assert r["S"] == sum(sp["hot"]) + sp["L"] == keys.size == int((bucket_of == b["d"]).sum())
        for k in ("NL", "chunks", "lsd_chunks", "peel_nl"):
            if k in sp:
                assert r[k] == sp[k], (k, r)
        # the bucket in arrival order is what the model was given
        assert np.array_equal(A.sort_keys(a.seed, a.ids[bucket_of == b["d"]]), keys)
        assert ((keys >> np.uint32(22)) == b["d"]).all(), "every stem of the bucket, light ones included, is in d"
        assert len(set(b["ids"].tolist())) == len(set(A.sort_keys(a.seed, b["ids"]).tolist())), "one stem per sort key"
        light = b["slots"] >= b["n_hot"]
        assert int(light.sum()) == sp["L"]
        for pos in (A.kbucket_positions(keys.size), A.peel_positions(keys.size)):
            assert pos.max() < keys.size
            lk = keys[pos][light[pos]]
            assert lk.size == 0 or np.unique(lk, return_counts=True)[1].max() < A.BK_HEAVY_MIN
        if sp["pairs"]:
            _, c = np.unique(keys[light], return_counts=True)
            assert (c == 2).sum() == sp["L"] // 2 and (c == 1).sum() == sp["L"] % 2
    # no other bucket is large, and every hot key crosses its limit inside one batch
    sizes = np.bincount(bucket_of, minlength=A.PART_DIGITS)
    aimed_d = [b["d"] for b in a.buckets]
    assert np.delete(sizes, aimed_d).max() <= 8
    assert (a.hot_limit < a.hot_total).all() and (a.hot_limit >= 1).all()
    assert set(np.unique(a.unit)) == {1, 2} and a.hits.min() == 0 and a.hits.max() == 8


def test_eleven_puts_both_buckets_in_one_walking_workgroup():
    d = [b["d"] for b in A.aimed("11").buckets]
    assert d[0] % A.BK_GRID == d[1] % A.BK_GRID and d[0] != d[1]
    assert [r["route"] for r in A.aimed("11").routes()] == ["P1", "P2-lsd"]


def test_placements_of_eight_and_nine():
    b = A.aimed("8").buckets[0]
    S = b["keys"].size
    assert list(A.kbucket_positions(S)[:3]) == [10, 30, 50] and list(A.peel_positions(S)[:2]) == [40, 120]
    assert (b["slots"][A.peel_positions(S)] == 0).all() and (b["slots"][A.kbucket_positions(S)] != 0).all()
    b = A.aimed("9").buckets[0]
    r = A.aimed("9").routes()[0]
    assert (b["slots"][A.kbucket_positions(b["keys"].size)] != 1).all()
    assert r["r"] == 1 and r["peel_r"] == 2 and r["NL"] > A.BIG_CAP >= r["peel_nl"]


def test_finder_returns_enough_stems_for_the_seeds_used():
    for d in (A.D_STAR, A.D_STAR ^ A.BK_GRID):
        ids, sk = A.find_ids(A.SEED, d, 4200)
        assert ids.size == 4200 and ids.max() < A.CANDIDATES and (np.diff(ids) > 0).all()
        assert ((sk >> np.uint32(22)) == d).all() and np.unique(sk).size == sk.size
        assert np.array_equal(A.sort_keys(A.SEED, ids), sk)
    with pytest.raises(ValueError):
        A.find_ids(A.SEED, A.D_STAR, 4200, limit=1 << 21)  # (about 2048 per bucket there)


def test_model_constants_match_the_source_text():
    src = open(os.path.join(CSRC, "rl_kernels.hip")).read()
    hdr = open(os.path.join(CSRC, "rl_kernels.h")).read()

    def const(text, name):
        m = re.findall(r"constexpr uint32_t %s = (\d+);" % name, text)
        assert len(m) == 1, name
        return int(m[0])

    assert const(src, "BK_HEAVY_MIN") == A.BK_HEAVY_MIN
    assert const(src, "BK_SAMPLES_PER_LANE") == A.BK_SAMPLES_PER_LANE
    assert const(hdr, "BIG_HEAVY") == A.BIG_HEAVY and "constexpr uint32_t BK_HEAVY = BIG_HEAVY;" in src
    assert const(src, "BK_GRID") == A.BK_GRID
    assert "using BkSmall = BkShape<%d, %d>;" % A.BK_SMALL in src and "using BkBig = BkShape<%d, %d>;" % A.BK_BIG in src
    assert "THREADS = 64 * W, CAP = 64 * W * IT" in src
    assert "constexpr uint32_t BIG_CHUNK = BkSmall::CAP;" in src and "constexpr uint32_t BIG_LIGHT_CAP = BkBig::CAP;" in src
    assert (A.SMALL_CAP, A.BIG_CAP, A.PART_DIGITS) == (2048, 4096, 1 << A.PART_BITS)
    # the two sample rules and the thresholds, as the kernels state them
    assert "(((uint64_t)(2 * (lane * R + i) + 1) * S) / (2 * NS))" in src and "NS = 64 * R" in src
    assert "(((uint64_t)(2 * lane + 1) * S) >> 7)" in src
    assert "if (S > B::CAP) {  // queued" in src and "if (M.r && nl <= BIG_LIGHT_CAP) {" in src
    assert "if (nl > B::CAP) return false;" in src and "if (NL > BIG_LIGHT_CAP) continue;" in src
    # the sort key is the hash's high word (but for k_run_check's one mark value, in the last bucket)
    assert "keys[i] = (uint32_t)(h >> 32) == KEY_DUP ? KEY_DUP - 1u : (uint32_t)(h >> 32);" in src
    assert "constexpr uint32_t KEY_DUP = 0xFFFFFFFFu;" in open(os.path.join(CSRC, "rl_device.h")).read()
    assert A.PART_DIGITS - 1 not in (A.D_STAR, A.D_STAR ^ A.BK_GRID)


def test_a_mutated_composition_changes_the_route():
    assert A.Aimed("4", L=4097).routes()[0]["route"] == "P2-lsd"
    r = A.Aimed("8", place=A._place_on_kbucket).routes()[0]
    assert r["route"] == "P1" and r["r"] == 1 and r["NL"] == 4020
    # and the model itself: a bucket at CAP is small, a key sampled twice is not heavy
    assert A.route(np.arange(2048, dtype=np.uint32))["route"] == "small"
    keys = np.arange(5120, dtype=np.uint32)
    keys[[10, 30]] = 7
    assert A.route(keys)["route"] == "P4"
    keys[50] = 7
    assert A.route(keys)["r"] == 1
