"""A CPU model of the counter table's slot discipline: open addressing, linear
probing, tombstones; no counters, no hash (a key's home slot is drawn at random
and kept with the key).

  insert   walks from the home slot, remembers the first tombstone on the path
           and claims it when it reaches an empty slot, else claims the empty
           slot. A probe window (max_probe slots) that ends without an empty
           slot: rule "parent" fails (the table's rule before reclamation
           existed, whatever lay on the path); rule "fixed" claims the
           remembered tombstone and fails only when the window held none.
  sweep    turns the given keys into tombstones. Under "fixed", when fewer than
           1 / RECLAIM_EMPTY_DIV of the slots are empty afterwards, every
           tombstone outside [home, slot) of all live keys becomes empty again.

The invariant both rules must keep (check_paths): no live key has an empty slot
between its home and its slot, or a lookup, which stops at the first empty slot,
would miss it.
"""
import functools

import numpy as np

EMPTY, TOMB, KEY = 0, 1, 2  # slot states
RECLAIM_EMPTY_DIV = 4  # (the library's SWEEP_RECLAIM_EMPTY_DIV)


class Table:
    def __init__(self, slots, rule="fixed", max_probe=None, reclaim="quarter"):
        """reclaim: "quarter" (the library's rule), "always" or "never"; under
        rule "parent" no sweep reclaims."""
        assert rule in ("parent", "fixed") and slots & (slots - 1) == 0
        self.n, self.rule, self.reclaim = slots, rule, reclaim
        self.max_probe = min(slots, 1 << 16) if max_probe is None else max_probe
        self.state = bytearray(slots)  # per slot EMPTY, TOMB or KEY (bytes: the walks are bytearray.find)
        self.key = [None] * slots      # the key of a KEY slot
        self.home = {}                 # key -> home slot
        self.at = {}                   # key -> its slot
        self.reclaims = 0

    # ---- counts
    def live(self):
        return len(self.at)

    def tombstones(self):
        return self.state.count(TOMB)

    def empties(self):
        return self.state.count(EMPTY)

    def _first(self, what, home, length):
        """The first slot in state `what` among the `length` slots from `home` on (wrapping), or -1."""
        end = home + length
        i = self.state.find(what, home, end)  # (an end past the table stops at the table's)
        if i < 0 and end > self.n:
            i = self.state.find(what, 0, end - self.n)
        return i

    # ---- the write path
    def insert(self, key, home):
        """True: the key has a slot (now or already); False: the table is full for it."""
        if key in self.at:
            return True
        e = self._first(EMPTY, home, self.max_probe)
        if e >= 0:  # the first tombstone on the path to the empty slot, else the empty slot
            t = self._first(TOMB, home, (e - home) % self.n)
            claim = t if t >= 0 else e
        elif self.rule == "fixed":  # the window ended: its first tombstone, if it has one
            claim = self._first(TOMB, home, self.max_probe)
        else:
            claim = -1
        if claim < 0:
            return False
        self.state[claim], self.key[claim] = KEY, key
        self.home[key], self.at[key] = home, claim
        return True

    def lookup(self, key, home):
        """The slot a probe finds the key in, or -1 (it stops at an empty slot or the window's end)."""
        i = home
        for _ in range(self.max_probe):
            if self.state[i] == EMPTY:
                return -1
            if self.state[i] == KEY and self.key[i] == key:
                return i
            i = (i + 1) & (self.n - 1)
        return -1

    def sweep(self, dead):
        """Tombstone the keys of `dead` that are live; returns how many."""
        k = 0
        for key in dead:
            i = self.at.pop(key, None)
            if i is not None:
                self.state[i], self.key[i] = TOMB, None
                del self.home[key]
                k += 1
        if self.rule == "fixed" and self.reclaim != "never":
            if self.reclaim == "always" or self.empties() * RECLAIM_EMPTY_DIV < self.n:
                self._reclaim()
        return k

    def _reclaim(self):
        n = self.n
        at = np.fromiter(self.at.values(), np.int64, len(self.at))
        home = np.fromiter((self.home[k] for k in self.at), np.int64, len(self.at))
        d = np.zeros(n + 1, np.int64)  # difference array of the ranges [home, slot), a wrapping one in two parts
        np.add.at(d, home, 1)
        np.add.at(d, at, -1)
        d[0] += int((home > at).sum())
        need = np.cumsum(d[:n]) > 0
        st = np.frombuffer(self.state, np.uint8)  # (a view: writes land in self.state)
        st[(st == TOMB) & ~need] = EMPTY
        self.reclaims += 1

    # ---- the probing invariant, slot by slot
    def check_paths(self):
        for key, at in self.at.items():
            h = self.home[key]
            dist = (at - h) % self.n
            assert dist < self.max_probe and self.state[at] == KEY and self.key[at] == key
            e = self._first(EMPTY, h, dist)
            assert e < 0, "key %d: empty slot %d between home %d and slot %d" % (key, e, h, at)


def churn(seed, slots=1024, live=512, keep=0.5, rounds=40, rule="fixed", reclaim="quarter", sweep_first=False,
          check=False, stop_on_fail=False):
    """Rounds of key turnover as a rate limiter's table sees them: every round
    `keep` of the live keys are hit again and the rest are replaced by keys never
    seen before (inserted one after another, random homes); a sweep drops the
    keys not hit. The sweep comes after the round's inserts (a batch, then
    rl_sweep at the batch's clock: the dead keys still hold their slots while
    the new ones arrive) or, with sweep_first, before them.
    -> (empties after each round's sweep, the first round in which an insert
    failed or None, the table). stop_on_fail ends the run at that round."""
    rng = np.random.default_rng(seed)
    t = Table(slots, rule, reclaim=reclaim)
    keys, next_key, empties, failed = [], 0, [], None
    for r in range(rounds):
        if keys:
            kept = set(rng.choice(len(keys), int(len(keys) * keep), replace=False).tolist())
            dead = [k for j, k in enumerate(keys) if j not in kept]
            keys = [k for j, k in enumerate(keys) if j in kept]
        else:
            dead = []
        if sweep_first:
            t.sweep(dead)
            if check:
                t.check_paths()
            empties.append(t.empties())
        for h in rng.integers(0, slots, live - len(keys)).tolist():
            if t.insert(next_key, h):
                keys.append(next_key)
            elif failed is None:
                failed = r
            next_key += 1
        if failed is not None and stop_on_fail:
            break
        if not sweep_first:
            t.sweep(dead)
            if check:
                t.check_paths()
            empties.append(t.empties())
    return empties, failed, t


BOUND_SEEDS, BOUND_ROUNDS, BOUND_FROM = 32, 40, 10


@functools.lru_cache(maxsize=None)
def min_empties_after_sweep():
    """The fewest empty slots after a sweep, rounds BOUND_FROM.. of BOUND_ROUNDS,
    in a 1024-slot table at 512 live keys with half of them replaced per round,
    over BOUND_SEEDS seeds of the fixed rules."""
    return min(min(churn(seed, rounds=BOUND_ROUNDS)[0][BOUND_FROM:]) for seed in range(BOUND_SEEDS))


def gpu_empties_bound():
    """What tests/test_gpu_churn.py asks of the GPU table per 1024 slots: half of
    the model's minimum. The GPU's inserts are concurrent (a lane that loses a
    tombstone takes a later slot) and its homes come from another hash; the
    factor 2 is the margin for both."""
    return min_empties_after_sweep() // 2
