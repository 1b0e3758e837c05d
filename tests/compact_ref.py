"""Plain reference of Compact (test infrastructure): the rule of DESIGN.md
4.9, literally, on a dump() dict.

Pure numpy/Python: no engine, no oracle library.  There is no reference
implementation to compare with (the reference never merges segments), so this
model IS the contract:

  Compact(fill_limit): while some pair of sibling leaves qualifies, merge it.
    siblings   two segments of one local depth L > initial_depth whose
               prefixes are 2q and 2q + 1 (adjacent in canonical order);
    qualifies  live(child 0) + live(child 1) <= fill_limit and the replay
               drops nothing;
    replay     the parent starts as child 0's image; e = the highest-index
               empty slot of child 1 (1023 if it has none); child 1's entries
               in the slot order e+1 .. 1023, 0 .. e go each to the first free
               slot of their 32-slot window (h & 0xFF) * 4 ..., cyclically; an
               entry whose window is full is a drop: the pair is refused and
               both children stay as they were.  The parent has depth L - 1
               and prefix q.

tests/test_compact_ref.py checks the model's properties on the CPU;
tests/test_gpu_compact.py checks the engine against the model.
"""
import numpy as np

from erase_ref import hash1
from limits_ref import INVALID, SLOTS, WINDOW


def replay(k0, v0, k1, v1):
    """Child 1 (k1, v1: lists of 1,024 Python ints) replayed into a copy of
    child 0 -> (keys, values) of the parent, or None if an entry is dropped."""
    pk, pv = list(k0), list(v0)
    e = SLOTS - 1
    while e > 0 and k1[e] != INVALID:
        e -= 1
    if k1[e] != INVALID:  # (no empty slot at all)
        e = SLOTS - 1
    for t in range(1, SLOTS + 1):
        s = (e + t) % SLOTS
        key = k1[s]
        if key == INVALID:
            continue
        w = (hash1(key) & 0xFF) * 4
        for d in range(WINDOW):
            j = (w + d) % SLOTS
            if pk[j] == INVALID:
                pk[j], pv[j] = key, v1[s]
                break
        else:
            return None
    return pk, pv


class CompactModel:
    """The segments of a dump() dict as a list of leaves [local depth, prefix,
    keys, values], in canonical order."""

    def __init__(self, dump, initial_depth):
        self.d0 = int(initial_depth)
        n = len(dump["local_depth"])
        k = np.asarray(dump["keys"], np.uint64).reshape(n, SLOTS)
        v = np.asarray(dump["values"], np.uint64).reshape(n, SLOTS)
        self.leaves = [[int(dump["local_depth"][i]), int(dump["prefix"][i]), k[i].tolist(), v[i].tolist()]
                       for i in range(n)]
        self.bad = set()  # (depth, prefix of child 0) of the pairs whose replay dropped: leaves that never change

    @staticmethod
    def live(leaf):
        return SLOTS - leaf[2].count(INVALID)

    def pairs(self, fill_limit):
        """Indices i of the sibling pairs (i, i + 1) within fill_limit that are not known to drop."""
        out = []
        for i in range(len(self.leaves) - 1):
            a, b = self.leaves[i], self.leaves[i + 1]
            if a[0] == b[0] and a[0] > self.d0 and a[1] % 2 == 0 and b[1] == a[1] + 1 and (a[0], a[1]) not in self.bad \
                    and self.live(a) + self.live(b) <= fill_limit:
                out.append(i)
        return out

    def merge(self, i):
        """Try pair (i, i + 1): True if merged, False if refused for a drop."""
        a, b = self.leaves[i], self.leaves[i + 1]
        r = replay(a[2], a[3], b[2], b[3])
        if r is None:
            self.bad.add((a[0], a[1]))
            return False
        self.leaves[i:i + 2] = [[a[0] - 1, a[1] >> 1, r[0], r[1]]]
        return True

    def image(self):
        ld = np.array([x[0] for x in self.leaves], np.uint32)
        return {"depth": max(self.d0, int(ld.max())), "local_depth": ld,
                "prefix": np.array([x[1] for x in self.leaves], np.uint64),
                "keys": np.array([x[2] for x in self.leaves], np.uint64).reshape(-1),
                "values": np.array([x[3] for x in self.leaves], np.uint64).reshape(-1)}


def _depth(m):
    return max(m.d0, max(x[0] for x in m.leaves))


def _result(m, before, depth_before, merges, rounds):
    return {"segments_before": before, "segments_after": len(m.leaves), "merges": merges, "refused": len(m.bad),
            "rounds": rounds, "depth_before": depth_before, "depth_after": _depth(m)}


def compact(dump, initial_depth, fill_limit=512):
    """Compact in bottom-up rounds: every round tries all the pairs the table
    shows, right to left so that indices stay valid.  -> (the new dump dict,
    the counts of pmdfc_compact_result_t).  A refused pair's leaves never
    change again, so `refused` counts pairs of the final table."""
    fill_limit = fill_limit or 512
    m = CompactModel(dump, initial_depth)
    before, depth_before = len(m.leaves), _depth(m)
    merges = rounds = 0
    while True:
        done = sum(m.merge(i) for i in reversed(m.pairs(fill_limit)))
        if not done:
            break
        merges += done
        rounds += 1
    return m.image(), _result(m, before, depth_before, merges, rounds)


def compact_random_order(dump, initial_depth, fill_limit, seed):
    """The same fixpoint reached one pair at a time, each picked at random."""
    rng = np.random.default_rng(seed)
    m = CompactModel(dump, initial_depth)
    before, depth_before = len(m.leaves), _depth(m)
    merges = 0
    while True:
        p = m.pairs(fill_limit or 512)
        if not p:
            break
        merges += m.merge(p[int(rng.integers(0, len(p)))])
    return m.image(), _result(m, before, depth_before, merges, None)
