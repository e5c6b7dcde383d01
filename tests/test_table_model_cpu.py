"""The counter table's slot discipline on the CPU model (tests/table_model.py):
what a table that never gets an empty slot back comes to under key turnover,
and that the fixed rules (a window that ends claims its first tombstone; a sweep
of a table short of empties frees the tombstones no live key needs) keep it
usable and keep every key findable. tests/test_gpu_churn.py asks the same of
the GPU table and takes its bound on the empty slots from here.

A "round of turnover" is a round that replaces keys: round 0 only fills the
table, so a failure in round r comes after r turnovers.
"""
import pytest

import table_model as M

SEEDS = range(32)


def test_model_parent_rule_runs_out_of_empties_under_full_turnover():
    """1024 slots, 512 live keys, every key replaced per round (the sweep first:
    512 old and 512 new keys do not fit side by side). Within 15 turnovers no
    empty slot is left and an insert fails, in a table that is half tombstones."""
    for seed in SEEDS:
        _, failed, t = M.churn(seed, keep=0.0, rounds=16, rule="parent", sweep_first=True, stop_on_fail=True)
        assert failed is not None and failed <= 15, (seed, failed)
        assert t.empties() == 0 and t.tombstones() > 0 and t.live() < 1024, seed
        assert not t.insert(1 << 40, seed)  # (and so does every later one, wherever its home)


def test_model_parent_rule_runs_out_of_empties_under_half_turnover():
    """Half of the 512 keys survive a round, the batch comes before the sweep:
    within 20 turnovers."""
    for seed in SEEDS:
        _, failed, t = M.churn(seed, keep=0.5, rounds=21, rule="parent", stop_on_fail=True)
        assert failed is not None and failed <= 20, (seed, failed)
        assert t.empties() == 0 and t.tombstones() > 0, seed
        assert not t.insert(1 << 40, seed)


@pytest.mark.parametrize("group", range(4))
def test_model_fixed_rules_never_fail_and_keep_every_path(group):
    """60 rounds for 32 seeds (8 per case), half and full turnover: no insert
    fails, and after every sweep no live key has an empty slot between its home
    and its slot (check_paths walks every key's path)."""
    for seed in range(8 * group, 8 * group + 8):
        empties, failed, t = M.churn(seed, keep=0.5, rounds=60, check=True)
        assert failed is None and t.live() == 512 and t.reclaims > 0, seed
    seed = 100 + group
    _, failed, t = M.churn(seed, keep=0.0, rounds=60, sweep_first=True, check=True)
    assert failed is None and t.live() == 512, seed


def test_model_window_end_claims_a_tombstone_and_full_means_full():
    """No empty slot at all: the fixed rule takes the first tombstone of the
    window, the parent's fails; with no tombstone either both fail."""
    for rule in ("parent", "fixed"):
        t = M.Table(64, rule, reclaim="never")
        for k in range(64):
            assert t.insert(k, 0)
        assert t.sweep([10, 20, 30]) == 3 and t.empties() == 0 and t.tombstones() == 3
        ok = t.insert(100, 15)
        assert ok == (rule == "fixed")
        if ok:
            assert t.at[100] == 20 and t.insert(101, 40) and t.at[101] == 10 and t.insert(102, 0) and t.at[102] == 30
            assert not t.insert(103, 0) and t.live() == 64
            t.check_paths()
    # a short window: only its own slots count
    t = M.Table(64, "fixed", max_probe=8, reclaim="never")
    for k in range(24):
        assert t.insert(k, 0 if k < 8 else 8) == (k < 16)  # (slots 0..7 from home 0, 8..15 from home 8)
    t.sweep([3])
    assert not t.insert(50, 4) and t.insert(50, 3) and t.at[50] == 3


def test_model_reclaim_frees_only_the_tombstones_no_key_needs():
    """Keys 0..9 homed at slot 0 sit in slots 0..9; with 1..8 dead, key 9 still
    needs slots 1..8 and key 0 nothing. A tombstone past every live key's slot
    is freed; a wrapping range is kept whole."""
    t = M.Table(32, "fixed", reclaim="always")
    for k in range(10):
        t.insert(k, 0)
    t.insert(20, 30), t.insert(21, 30), t.insert(22, 30), t.insert(23, 30)  # slots 30, 31, then 10, 11 (wrapped)
    assert [t.at[k] for k in (20, 21, 22, 23)] == [30, 31, 10, 11]
    t.sweep([1, 2, 3, 4, 5, 6, 7, 8, 20, 21, 22])
    # key 9 needs [0, 9); key 23 (home 30, slot 11) needs 30, 31 and 0..10
    assert t.tombstones() == 11 and t.empties() == 32 - 3 - 11
    t.check_paths()
    t.sweep([23])
    assert t.tombstones() == 8 and t.lookup(9, 0) == 9
    t.sweep([9])
    assert t.tombstones() == 0 and t.empties() == 31 and t.lookup(0, 0) == 0


def test_model_bound_for_the_gpu_test():
    """The fewest empties after a sweep from round 10 on (512 of 1024 slots, half
    turnover, batch before sweep, 32 seeds x 40 rounds) is 153 slots with
    numpy's default_rng; the GPU test asks for half of it, 76 per 1024 slots.
    Pinned loosely: any reclamation worth the name leaves well over a tenth of
    the table empty, and cannot leave more than the 512 slots no key holds."""
    lo = M.min_empties_after_sweep()
    assert 1024 // 10 < lo <= 512, lo
    assert M.gpu_empties_bound() == lo // 2
    # without reclamation the same run has no empty slot left long before round 40
    e, failed, _ = M.churn(0, rounds=40, reclaim="never")
    assert failed is None and min(e[10:]) < lo // 2  # (the fixed insert rule alone keeps inserts working)
