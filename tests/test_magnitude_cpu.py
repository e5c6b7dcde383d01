"""The references at the top of the u32 range, on the CPU.

tests/test_gpu_magnitude.py compares the engine with the C oracle (and, on
single-unit streams, with magnitude.ExactModel) on limits, addends and counts
up to 2^32 - 1 and on clocks at both ends of the accepted range. This file
proves, without a GPU, that those references agree with each other on the very
streams the GPU file runs (magnitude.stream returns the same objects), on the
decide grid, on hand-computed answers and on random call streams around 2^31
and 2^32 - 128; and that every stream stays inside the budget: the model raises
(OutOfModel) if a count would pass 2^32 - 1 or a u32 subtraction of the Go code
would go below zero."""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import oracle as O
from ratelimit_amd.packing import RuleInterner, pack_calls
import magnitude as M
import streams

# streams small enough for the pure-Python oracle to join (it takes calls: one per request)
PY_TOO = ("short", "exact", "history_second", "history_minute", "zero_units", "top", "counted")
CASES = [(name, ep) for name in M.STREAMS for ep in (["now0"] if name in M.EPOCH_FREE else list(M.CLOCK_EPOCHS))]


@pytest.mark.parametrize("lc", [False, True])
@pytest.mark.parametrize("name,epoch", CASES)
def test_model_and_oracles_agree_on_the_gpu_streams(name, epoch, lc):
    bs = M.oracle_input(name, M.stream(name, epoch))
    want, model = M.reference(name, epoch, lc)  # (the model did not raise: no count reached 2^32)
    for k, (w, m) in enumerate(zip(want, model)):
        for f in M.FIELDS:
            assert np.array_equal(w[f], m[f]), M.explain(w, m, m, bs[k][0], bs[k][1], "batch %d, C oracle vs model:" % k)
    if name in PY_TOO:
        py, oc = M.python_oracle_packed(bs, 0.8, lc)
        for k, (w, p) in enumerate(zip(want, py)):
            for f in M.FIELDS:
                assert np.array_equal(w[f], p[f]), M.explain(w, p, model[k], bs[k][0], bs[k][1],
                                                             "batch %d, C vs Python oracle:" % k)
    if name != "counted":
        M.coverage(name, bs, model, lc)
    for a, n, nq, nr in bs:  # the clocks are where the epoch says
        assert a["now"].min() >= 0 and a["now"].max() <= M.NOW_MAX
    if epoch == "top":
        assert max(int(b[0]["now"].max()) for b in bs) >= M.NOW_MAX - 2
    if epoch == "zero" or name == "zero_units":
        assert min(int(b[0]["now"].min()) for b in bs) == 0


def test_top_stream_refuses_one_request_only():
    bs = M.stream("top")
    a, n, nq, nr = bs[1]
    assert int((a["now"] > M.NOW_MAX).sum()) == 1 and a["now"][M.TOP_BAD] == M.NOW_MAX + 1
    assert 0 < M.TOP_BAD < nq - 1 and int((~M.top_keep(bs[1])).sum()) == 2
    assert (np.delete(a["now"], M.TOP_BAD) == M.NOW_MAX).all() and (a["unit"] == 4).all()


def test_crossing_runs_cross_where_they_say():
    """The crossing generator: the chosen element of a hot run is the first
    OVER_LIMIT one, the element before it is OK above near, and with a limit
    at the top before and after are above 2^31."""
    rng = np.random.default_rng(1)
    hot = np.arange(6)
    ten = rng.permutation(np.r_[np.repeat(hot, [40, 40, 40, 5, 5, 5]), 100 + np.arange(50)])
    b1, b2, mask = M.crossing_runs(ten, hot, 1000, rng, [2 ** 31 + 1, 2 ** 32 - 1], ("first", "mid", "last"))
    m1, m2 = M.exact_model([b1, b2])
    assert (m1["code"] == M.OK).all()
    for i, t in enumerate(hot.tolist()):
        pos = 2 * np.nonzero(ten == t)[0]  # the sec descriptors of the run
        c = {0: 0, 1: len(pos) // 2, 2: len(pos) - 1}[i % 3]
        codes = m2["code"][pos]
        assert (codes[:c] == M.OK).all() and (codes[c:] == M.OVER).all(), (t, codes)
        near = M.near_threshold(int(b2[0]["limit"][pos[0]]), 0.8)
        assert m2["before"][pos[0]] < near < m2["after"][pos[0]]
        if i % 2:  # the top limit
            assert m2["before"][pos[c]] > 2 ** 31 and b2[0]["limit"][pos[0]] == 2 ** 32 - 4096


# --------------------------------------------------------------------------- the decide grid
@pytest.mark.parametrize("ratio", [0.8, 1.0])
def test_decide_grid_python_oracle_vs_exact_model(ratio):
    """GetResponseDescriptorStatus of the Python oracle (u32, masked) against the
    model's decide (exact) on before x hits x limit x shadow x local-cache hit,
    the local cache on and off. Where the model steps outside exact integers it
    must be for the one documented reason: at ratio 1.0 float32(limit) rounds
    above the limit (2^31 - 1, 2^32 - 2, 2^32 - 1), so limit - near wraps in Go;
    those cases are left to the oracle-vs-oracle test below."""
    outside = 0
    grid = M.decide_grid()
    assert len(grid) > 1500
    for lc_en in (False, True):
        for case in grid:
            before, after, lc_hit, h, limit, shadow = case
            got = M.python_decide(ratio, lc_en, case)
            try:
                want = M.decide(before, after, lc_hit, h, limit, ratio, shadow, lc_en)
            except M.OutOfModel:
                assert ratio == 1.0 and float(np.float32(limit)) > limit, case
                outside += 1
                continue
            assert got == (want[0], want[1], want[2], want[3]), (ratio, lc_en, case, got, want)
    assert (outside > 0) == (ratio == 1.0) and outside < len(grid) // 4


@pytest.mark.parametrize("ratio", [0.8, 1.0, 1.25])
def test_decide_grid_c_oracle_vs_python_oracle(ratio):
    """The two oracles on the grid (ratio 1.25 wraps in u32 by design and is
    outside the model): the C oracle is driven through restore (count = before)
    and one DoLimit of `hits` per key."""
    cases = [c for c in M.decide_grid() if not c[2]]
    n = len(cases)
    stems = [b"grid_case_%d_" % i for i in range(n)]
    co = c_oracle.COracle(ratio, False)
    seeded = [i for i, c in enumerate(cases) if c[0]]
    co.restore([stems[i] for i in seeded], [2] * len(seeded), [0] * len(seeded), [cases[i][0] for i in seeded])
    from ratelimit_amd.packing import arrays_from_lists
    a = arrays_from_lists(stems, [0] * n, list(range(n)), [2] * n, [1 if c[5] else 0 for c in cases],
                          [c[4] for c in cases], [c[3] for c in cases], list(range(n)))
    o = co.do_limit(a, n, n, n)
    co.close()
    st = o["stats"].reshape(n, 6)
    for i, c in enumerate(cases):
        code, rem, deltas, _ = M.python_decide(ratio, False, c)
        assert (int(o["code"][i]), int(o["limit_remaining"][i])) == (code, rem), (ratio, c)
        assert tuple(int(x) for x in st[i, 1:]) == deltas[1:] and st[i, 0] == c[3], (ratio, c, st[i], deltas)


# --------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("lc", [False, True])
def test_known_answers_model_and_both_oracles(lc):
    cases = M.golden_cases()
    assert len(cases) >= 20 and all(c["why"] for c in cases)
    steps = M.golden_batches(cases, lc)
    bs = [s[0] for s in steps]
    co = c_oracle.COracle(0.8, lc)
    c_out = [co.do_limit(*b) for b in bs]
    co.close()
    py_out, _ = M.python_oracle_packed(bs, 0.8, lc)
    mo_out = M.exact_model(bs, 0.8, lc)
    for k, (b, expect, names) in enumerate(steps):
        for who, out in (("C oracle", c_out), ("Python oracle", py_out), ("model", mo_out)):
            got = list(zip(out[k]["code"].tolist(), out[k]["limit_remaining"].tolist()))
            assert got == expect, (who, k, [(nm, g, e) for nm, g, e in zip(names, got, expect) if g != e])


# --------------------------------------------------------------------------- random call streams
@pytest.mark.parametrize("where,seed", M.RANDOM_CASES)
@pytest.mark.parametrize("lc", [False, True])
def test_random_streams_around_the_sign_bit_and_the_top(where, seed, lc):
    """Structured call streams (overrides, shadow rules, duplicates, hits 0)
    whose limits lie around 2^31 and around 2^32 - 128, every key primed to just
    below them: Python oracle == C oracle == model, and the budget
    (random_worst after the priming) keeps every count of the oracle's store
    at or below 2^32 - 1."""
    n_calls, limit_range, prime = M.RANDOM_RANGES[where]
    assert prime + M.random_worst(n_calls) <= M.U32_MAX
    calls = M.primed_stream(seed, limit_range, prime, n_calls=n_calls, zipf=seed % 2 == 0, **M.RANDOM_KW)
    assert max(r.hits_addend for r, _, _ in calls[-n_calls:]) <= M.RANDOM_MAX_ADDEND
    assert max(len(r.descriptors) for r, _, _ in calls) <= M.RANDOM_MAX_DESC
    streams.reset_stats(calls)
    oc = O.OracleFixedRateLimitCache(0.8, lc)
    py = [oc.do_limit(r, l, now) for r, l, now in calls]
    added = {}
    for op, key, h in oc.client.log:  # (INCRBY sums bound every count the store ever held)
        if op == "INCRBY":
            added[key] = added.get(key, 0) + h
    assert max(added.values()) <= M.U32_MAX and max(e[0] for e in oc.client.data.values()) <= M.U32_MAX
    assert max(added.values()) > prime
    interner = RuleInterner()
    pb = pack_calls(calls, "", interner)
    nr = len(interner.keys)
    co = c_oracle.COracle(0.8, lc)
    c = co.do_limit(pb.arrays, pb.n, pb.n_requests, nr)
    co.close()
    m, = M.exact_model([(pb.arrays, pb.n, pb.n_requests, nr)], 0.8, lc)
    for f in M.FIELDS:
        assert np.array_equal(c[f], m[f]), M.explain(c, m, m, pb.arrays, pb.n, "C oracle vs model:")
    for j, (ci, di) in enumerate(pb.origin):
        s = py[ci][di]
        assert (s.code, s.limit_remaining, s.duration_until_reset) == (c["code"][j], c["limit_remaining"][j],
                                                                       c["reset_s"][j]), (ci, di)
    py_stats = {}
    for _, limits, _ in calls:
        for l in limits:
            if l is not None:
                py_stats[l.stats.key] = l.stats.as_tuple()
    got = {k: tuple(int(x) for x in c["stats"][i * 6:i * 6 + 6]) for i, k in enumerate(interner.keys)}
    assert got == py_stats
    assert (c["code"] == M.OK).any() and (c["code"] == M.OVER).any(), (where, seed)


def test_c1_batch_dev_keeps_wide_hits_on_the_cpu():
    """workloads.c1_batch_dev with torch on the CPU: the int32 tensors hold the
    bits of c1_batch's uint32 arrays for addends up to 2^32 - 1 (the GPU file
    repeats this on the device)."""
    from ratelimit_amd import workloads as W
    t = np.arange(7)
    h = np.array(M.HITS_EDGES, np.uint32)
    a, n, nq, nr = W.c1_batch(t, M.NOW_MAX, h)
    for hits in (h, h.astype(np.int64).tolist()):
        d, dn, dq, dr = W.c1_batch_dev(t, M.NOW_MAX, hits, device="cpu")
        assert (dn, dq, dr) == (n, nq, nr)
        for k, v in a.items():
            got = d[k].numpy()
            assert np.array_equal(got.view(v.dtype) if got.dtype != v.dtype else got, v), k
