"""The maintenance-mix plan (tests/maintenance_mix.py) proven on the CPU, with
the oracle alone: the schedule covers every ordered pair of calls, the walks
stay in the planned ranges, every step is felt by the stream that follows it,
and every checker fails on a reader with the defect it is there to find. What
holds here holds for tests/test_gpu_maintenance_mix.py, which makes the same
calls in the same order."""
import pytest

import maintenance_mix as M
from oracle import oracle as O

_done = {}


def walked(k):
    """Walk k driven to its end with the oracle alone (once per walk): -> (walk, per-step reports)."""
    if k not in _done:
        wk, steps = M.Walk(k), []
        wk.segment(0)
        for i, op in enumerate(wk.ops):
            a = wk.args(i)
            rep = dict(op=op, args=a, live=len(wk.model), now=wk.now, floor_before=wk.floor)
            rep["n"] = wk.apply(i, a)
            rep.update(slots=wk.slots, history=wk.history, shards=wk.shards, late_reads=wk.late_reads)
            steps.append(rep)
            wk.segment(i + 1)
        _done[k] = (wk, steps)
    return _done[k]


def test_the_circuit_covers_every_ordered_pair():
    c = M.euler_circuit()
    assert len(c) == 101 and c[0] == c[-1]
    assert sorted(zip(c, c[1:])) == sorted((a, b) for a in M.OPS for b in M.OPS)
    pairs = []
    for k in range(4):
        ops = M.walk_ops(k)
        assert len(ops) == 26
        pairs += list(zip(ops, ops[1:]))
    assert sorted(pairs) == sorted((a, b) for a in M.OPS for b in M.OPS)  # 100 pairs, each once, none in a cut
    table = M.pair_table()
    print(table)
    cells = [c for row in table.splitlines()[1:] for c in row.split()[1:]]
    assert len(cells) == len(set(cells)) == 100  # every pair at a step of its own


def test_the_stream_has_the_kinds_and_late_calls():
    seg = M.mix_stream(100, 27)
    calls = [c for s in seg for c in s]
    assert len(seg[0]) >= M.PRELUDE_CALLS and all(M.SEG_CALLS <= len(s) <= M.SEG_CALLS + 2 for s in seg[1:])
    run, late = M.START, []
    for r, lims, now in calls:
        if M.START < now < run:  # (a late call in the stream's first seconds stops at its start)
            late.append((run - now, lims[0].limit.unit))
            assert len(lims) == 1
        run = max(run, now)
    assert len(late) > 300
    assert {d for d, u in late if u == O.SECOND} == set(range(1, 8))
    assert {d for d, u in late if u == O.MINUTE} == {60, 120, 180}
    assert all(u in (O.SECOND, O.MINUTE) for _, u in late) and max(d for d, _ in late) < M.LAG
    # the prelude spans more than the lag (the first step may be a sweep), and no walk reaches the next hour
    # (a stem under MINUTE and HOUR shares a Redis key between its units there: test_gpu_alias's subject)
    assert seg[0][-1][2] - M.START > M.LAG + 120
    assert run < M.START - M.START % 3600 + 3600


@pytest.mark.parametrize("k", range(4))
def test_the_plan_stays_in_range(k):
    wk, steps = walked(k)
    assert [s["op"] for s in steps] == M.walk_ops(k)
    assert all(s["slots"] in M.SLOTS and s["history"] in (M.H_FLOOR, 4 * M.H_FLOOR) and s["shards"] in (1, 2)
               for s in steps)
    assert {s["slots"] for s in steps} == set(M.SLOTS) and {s["shards"] for s in steps} == {1, 2}
    assert max(s["live"] for s in steps) <= 512  # a table of 2^10 slots (max_probe 1024) takes them all
    # the log: an upper estimate of history_appended summed over the walk's ctxs, below one partition's size
    print("walk", k, "appends", wk.appends, sum(wk.appends), "late reads", wk.late_reads, "calls", wk.tick)
    assert sum(wk.appends) < M.H_FLOOR // 64 == 8192
    assert wk.late_reads >= len(steps)  # (one a step on average; that every step has one: the feltness tests)
    for s in steps:
        if s["op"] in ("F_KEYS", "F_PREFIX"):
            assert s["n"] > 0, (k, s)
        if s["op"] == "F_PREFIX":
            assert len(s["args"][1]) > 36  # (ends inside a long stem's arena part)
        if s["op"] == "SWEEP":
            assert s["n"] > 0 and s["args"] > s["floor_before"], (k, s)


@pytest.mark.parametrize("k", range(4))
def test_every_deletion_is_felt(k):
    """The rest of the walk without that one deletion: some answer changes."""
    wk, steps = walked(k)
    n = 0
    for i, s in enumerate(steps):
        if s["op"] in ("F_KEYS", "F_PREFIX"):
            oc, _ = wk.snaps[i]
            assert wk.replay(M.clone(oc), i) is not None, (k, i, s["op"], s["args"])
            n += 1
    assert n >= 2


@pytest.mark.parametrize("k", range(4))
def test_every_state_preserving_step_is_felt(k):
    """An oracle that loses the older-than-newest windows at that step answers
    differently before the next such step: a late call reads, after every
    step, a window written before it."""
    wk, steps = walked(k)
    nxt = len(steps)
    for i in range(len(steps) - 1, -1, -1):
        if steps[i]["op"] not in M.PRESERVING:
            continue
        oc, model = wk.snaps[i]
        oc = M.clone(oc)
        assert M.without_older_windows(wk, oc, model) > 0
        assert wk.replay(oc, i, until=nxt) is not None, (k, i, steps[i]["op"])
        nxt = i


@pytest.mark.parametrize("k", (0, 2))
def test_the_local_cache_is_felt_across_each_kind_of_step(k):
    wk, steps = walked(k)
    felt = set()
    for i, s in enumerate(steps):
        if s["op"] in M.PRESERVING:
            oc = M.clone(wk.snaps[i][0])
            oc.local_cache.data.clear()
            if wk.replay(oc, i) is not None:
                felt.add(s["op"])
    assert felt == set(M.PRESERVING)


# --------------------------------------------------------------------------- the checkers can fail
def _mid_walk():
    """Walk 0 stopped after a step that follows a sweep and a deletion, its readers faked from the oracle."""
    wk = M.Walk(0)
    wk.segment(0)
    for i, op in enumerate(wk.ops):
        wk.apply(i, wk.args(i))
        if wk.floor and wk.deleted and i >= 8:
            return wk
        wk.segment(i + 1)
    raise AssertionError("no such step")


def test_the_checkers_pass_on_a_faithful_reader_and_fail_on_each_defect():
    wk = _mid_walk()
    rd = M.FakeReader(wk)
    export = M.check_readers(rd, wk)
    assert M.check_export(export, wk) > 20                      # live keys compared
    assert M.check_hot(rd, export, wk) > 0 and M.check_hot(rd, export, wk, blocked=True) > 0
    probes, found = M.check_lookup(rd, wk)
    assert probes >= 40 and found >= 10 and wk.floor > 0
    for defect, check in (
            ("forgotten_kept", lambda r: M.check_export(r.export(), wk)),
            ("older_dropped", lambda r: M.check_export(r.export(), wk)),
            ("count_off", lambda r: M.check_export(r.export(), wk)),
            ("scan_older_dropped", lambda r: M.check_scans(r, export, wk)),
            ("floor_zero", lambda r: M.check_scans(r, export, wk)),
            ("hot_off", lambda r: M.check_hot(r, export, wk)),
            ("lookup_off", lambda r: M.check_lookup(r, wk))):
        with pytest.raises(AssertionError):
            check(M.FakeReader(wk, defect))
        with pytest.raises(AssertionError):
            M.check_readers(M.FakeReader(wk, defect), wk)
    # table_info: a slot too many, a tombstone after a resize, a lost entry, another size
    info = rd.table_info()
    wk.tomb_zero = True
    M.check_table_info(info, export, wk, exact_arena="live")
    for f in ("live_slots", "tombstones", "history_lost", "history_refused", "history_entries", "table_slots",
              "arena_bytes_used"):
        with pytest.raises(AssertionError):
            M.check_table_info(dict(info, **{f: info[f] + 1}), export, wk, exact_arena="live")
    with pytest.raises(AssertionError):
        M.check_table_info(dict(info, arena_bytes_used=info["arena_bytes_used"] - 16), export, wk)


def test_the_op_checks_fail_on_a_wrong_count():
    """check_op against exports taken around a deletion and a sweep of the oracle's own."""
    import numpy as np
    wk = M.Walk(0)
    wk.segment(0)
    seen = set()
    for i, op in enumerate(wk.ops):
        a = wk.args(i)
        rd = M.FakeReader(wk)
        pre, ia = rd.export(), dict(rd.table_info(), history_appended=0, history_slots=0)
        units = {}
        for r in pre:
            units.setdefault(r[0], set()).add(r[1])
        wk.apply(i, a)
        post, ib = rd.export(), dict(rd.table_info(), history_appended=0, history_slots=0)
        if op in ("F_KEYS", "F_PREFIX") and op not in seen:
            hit = lambda s, p: s == p if op == "F_KEYS" else s.startswith(p)
            removed = [sum(len(u) for s, u in units.items() if hit(s, p) and not any(hit(s, q) for q in a[:j]))
                       for j, p in enumerate(a)]
            gone = [s for s in units if any(hit(s, p) for p in a)]
            got = dict(removed=np.array(removed), keys=sum(removed), keys_with_history=sum(removed),
                       arena_bytes=sum(M.arena_bytes(s) * len(units[s]) for s in gone),
                       slots_scanned=wk.shards * wk.slots if op == "F_PREFIX" else 0)
            ia["tombstones"], ib["tombstones"] = 0, got["keys"]
            ib["arena_bytes_used"] = ia["arena_bytes_used"]
            M.check_op(op, a, got, pre, ia, post, ib, wk)
            with pytest.raises(AssertionError):
                M.check_op(op, a, dict(got, keys=got["keys"] + 1), pre, ia, post, ib, wk)
            with pytest.raises(AssertionError):
                M.check_op(op, a, got, pre, ia, pre, ib, wk)  # (nothing was removed)
            seen.add(op)
        if op == "SWEEP" and op not in seen:
            n = len(M.expired_keys(pre, a))
            assert n > 0
            M.check_op(op, a, n, pre, ia, post, ib, wk)
            with pytest.raises(AssertionError):
                M.check_op(op, a, n - 1, pre, ia, post, ib, wk)
            with pytest.raises(AssertionError):
                M.check_op(op, a, n, pre, ia, pre, ib, wk)
            seen.add(op)
        wk.segment(i + 1)
    assert seen == {"F_KEYS", "F_PREFIX", "SWEEP"}
