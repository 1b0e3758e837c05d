"""Plain reference of Erase (test infrastructure): the serial rule of
DESIGN.md 4.8, literally, on the table model of tests/limits_ref.py.

Pure numpy/Python: no engine, no oracle library.  There is no reference
implementation to compare with (the reference's Delete is a stub), so this
model IS the contract:

  Erase(key): repeat until the probe misses --
    1. probe the key's 32-slot window in probe order up to the first empty
       slot; no match: stop;
    2. p = the first match;
    3. backward shift: among the slots p+1 .. p+31 (cyclic) up to the first
       empty one, take the first entry c whose own window start lies at or
       before p, (c - w_c) mod 1024 >= (c - p) mod 1024; copy pair c to p, set
       p = c, look again; when there is none, write {INVALID, 0} at p.

tests/test_erase_ref.py checks the model's properties on the CPU;
tests/test_gpu_erase.py checks the engine against the model;
tests/test_churn_ref.py holds the serial oracle's restatement (oc_erase) to it.
"""
import numpy as np

from limits_ref import INVALID, SENTINEL, SLOTS, ST_MISS, ST_RESERVED_KEY, WINDOW, FrozenTable, hash64

ST_ERASED = 12
_M64 = (1 << 64) - 1
_MUL = 0xc6a4a7935bd1e995


def hash1(key: int) -> int:
    """hash64 of one key in Python ints (the shift hashes every entry it looks at)."""
    d = (key * _MUL) & _M64
    d = ((d ^ (d >> 47)) * _MUL) & _M64
    h = (0xc70697 ^ ((8 * _MUL) & _M64)) ^ d
    h = (h * _MUL) & _M64
    h = ((h ^ (h >> 47)) * _MUL) & _M64
    return h ^ (h >> 47)


class ErasableTable(FrozenTable):
    """FrozenTable with Erase.  max_chain / moves: the longest shift chain of
    one removed copy and the entries moved in all (reported by the tests)."""

    def __init__(self, dump, upsert=False):
        super().__init__(dump, upsert)
        self.max_chain = 0
        self.moves = 0

    def _erase(self, s, h, key):
        if key >= SENTINEL:
            return ST_RESERVED_KEY
        rk, rv = self._k[s], self._v[s]
        w = (h & 0xFF) * 4
        erased = False
        for _ in range(WINDOW + 1):  # (a window holds 32 copies at most)
            # 1. the window in probe order up to its first empty slot
            p = None
            for t in range(WINDOW):
                j = (w + t) % SLOTS
                if rk[j] == INVALID:
                    break
                if rk[j] == key:
                    p = j  # 2. the first match
                    break
            if p is None:
                return ST_ERASED if erased else ST_MISS
            erased = True
            # 3. backward shift
            chain = 0
            while True:
                c = None
                for d in range(1, WINDOW):
                    j = (p + d) % SLOTS
                    if rk[j] == INVALID:
                        break
                    wc = (hash1(rk[j]) & 0xFF) * 4
                    if (j - wc) % SLOTS >= d:
                        c = j
                        break
                if c is None:
                    rk[p], rv[p] = INVALID, 0
                    break
                rk[p], rv[p] = rk[c], rv[c]
                p = c
                chain += 1
                assert chain <= SLOTS, "the shift does not end"
            self.max_chain = max(self.max_chain, chain)
            self.moves += chain
        raise AssertionError("more than 32 copies of a key in one window")

    def erase(self, key) -> int:
        """One Erase -> ST_ERASED (one or more copies removed), ST_MISS, ST_RESERVED_KEY."""
        h = hash64(np.array([key], np.uint64))
        return self._erase(int(self._segments(h)[0]), int(h[0]), int(key))

    def erase_batch(self, keys) -> np.ndarray:
        """The keys erased one by one, in order -> statuses, as CCEH.Erase returns them."""
        keys = np.ascontiguousarray(keys, np.uint64)
        h = hash64(keys)
        seg = self._segments(h).tolist()
        return np.array([self._erase(s, hh, k) for s, hh, k in zip(seg, h.tolist(), keys.tolist())], np.uint8)

    def live(self) -> int:
        return sum(SLOTS - row.count(INVALID) for row in self._k)

    def copies(self, key):
        """The values stored under `key`, in probe order."""
        h = int(hash64(np.array([key], np.uint64))[0])
        s = int(self._segments(np.array([h], np.uint64))[0])
        w = (h & 0xFF) * 4
        out = []
        for t in range(WINDOW):
            j = (w + t) % SLOTS
            if self._k[s][j] == INVALID:
                break
            if self._k[s][j] == int(key):
                out.append(self._v[s][j])
        return out


def erase_plan(stream_keys, seed, n_absent=300):
    """What the tests erase from a table built from a stream: a seeded half of
    its distinct keys, n_absent keys it never held and the two reserved keys,
    shuffled.  -> (erase keys in order, the distinct keys that stay)."""
    rng = np.random.default_rng(seed)
    distinct = np.unique(np.asarray(stream_keys, np.uint64))
    distinct = distinct[distinct < np.uint64(SENTINEL)]
    gone = rng.random(distinct.size) < 0.5
    absent = rng.integers(1, 1 << 63, n_absent, dtype=np.uint64) | np.uint64(1 << 63)
    absent = absent[~np.isin(absent, distinct) & (absent < np.uint64(SENTINEL))]
    plan = np.concatenate([distinct[gone], absent, np.array([INVALID, SENTINEL], np.uint64)])
    return plan[rng.permutation(plan.size)], distinct[~gone]
