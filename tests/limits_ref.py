"""Plain reference of a table that cannot split (test infrastructure).

Pure numpy/Python: no engine, no oracle library.  Once the arena or the
sub-directory pool is exhausted the engine answers PMDFC_ST_CAPACITY and stops
splitting; from then on the table is a fixed set of segments, and the serial
answer of any batch follows from the dump alone:

  FrozenTable       applies ops serially to a dump() dict with no split: the
                    exact answer of every batch across which nothing split;
  check_table       the structure every valid table has, whatever happened;
  check_accounting  what is stored is exactly what was answered INSERTED.

tests/test_limits_ref.py checks the model against the serial oracle;
tests/test_gpu_limits.py checks the engine against the model.
"""
import numpy as np

INVALID = 0xFFFFFFFFFFFFFFFF
SENTINEL = INVALID - 1
SLOTS, WINDOW = 1024, 32
(ST_MISS, ST_HIT, ST_INSERTED, ST_RESERVED_KEY, ST_UNSPLITTABLE, ST_DEPTH_LIMIT, ST_CAPACITY) = range(7)
ST_UPDATED = 11
OP_GET, OP_INSERT = 0, 1


def hash64(keys) -> np.ndarray:
    """std::_Hash_bytes(&key, 8, 0xc70697) in numpy (csrc/cceh_device.h hash64)."""
    mul, s47 = np.uint64(0xc6a4a7935bd1e995), np.uint64(47)
    with np.errstate(over="ignore"):
        d = np.ascontiguousarray(keys, dtype=np.uint64) * mul
        d = (d ^ (d >> s47)) * mul
        h = np.uint64(0xc70697 ^ ((8 * 0xc6a4a7935bd1e995) & INVALID)) ^ d
        h = h * mul
        h = (h ^ (h >> s47)) * mul
        return h ^ (h >> s47)


def _starts(local_depth, prefix):
    """First hash of each segment's range: prefix << (64 - local depth)."""
    ld = np.asarray(local_depth, np.uint64)
    px = np.asarray(prefix, np.uint64)
    return np.where(ld == 0, np.uint64(0), px << (np.uint64(64) - np.maximum(ld, np.uint64(1))))


class FrozenTable:
    """The serial table of CCEH_hybrid with Segment::Split taken away, built
    from a dump() dict (depth, local_depth, prefix, keys, values; segments in
    directory order).  The segment of a key is the one whose prefix its hash
    h starts with; its window is the 32 slots from (h & 0xFF) * 4 on, wrapping
    at 1024."""

    def __init__(self, dump, upsert=False):
        self.depth = int(dump["depth"])
        self.local_depth = np.array(dump["local_depth"], np.uint32)
        self.prefix = np.array(dump["prefix"], np.uint64)
        self.upsert = bool(upsert)
        n = self.local_depth.size
        starts = _starts(self.local_depth, self.prefix)
        assert np.all(starts[1:] > starts[:-1]) and (n == 0 or starts[0] == 0), "segments not in directory order"
        self._starts = starts
        k = np.asarray(dump["keys"], np.uint64).reshape(n, SLOTS)
        v = np.asarray(dump["values"], np.uint64).reshape(n, SLOTS)
        self._k = [row.tolist() for row in k]  # Python ints: list.index scans a window at C speed
        self._v = [row.tolist() for row in v]

    def _segments(self, h):
        return np.searchsorted(self._starts, h, side="right") - 1

    @staticmethod
    def _window(row, w):
        return row[w:w + WINDOW] if w + WINDOW <= SLOTS else row[w:] + row[:w + WINDOW - SLOTS]

    def _insert(self, s, h, key, value):
        if key >= SENTINEL:
            return ST_RESERVED_KEY
        w = (h & 0xFF) * 4
        win = self._window(self._k[s], w)
        j = win.index(INVALID) if INVALID in win else WINDOW
        st = ST_INSERTED
        if self.upsert and key in win and win.index(key) < j:
            j, st = win.index(key), ST_UPDATED
        if j == WINDOW:
            # every entry carries the key's full hash (hash64 is a bijection:
            # every entry is the key): a split could never separate them
            return ST_UNSPLITTABLE if all(x == key for x in win) else ST_CAPACITY
        p = (w + j) % SLOTS
        self._k[s][p] = key
        self._v[s][p] = value
        return st

    def _get(self, s, h, key):
        if key >= SENTINEL:
            return 0, ST_RESERVED_KEY
        w = (h & 0xFF) * 4
        win = self._window(self._k[s], w)
        if key in win:
            return self._v[s][(w + win.index(key)) % SLOTS], ST_HIT
        return 0, ST_MISS

    def insert(self, key, value=1) -> int:
        """One Insert; the table changes only if it answers INSERTED / UPDATED."""
        h = hash64(np.array([key], np.uint64))
        return self._insert(int(self._segments(h)[0]), int(h[0]), int(key), int(value))

    def get(self, key):
        h = hash64(np.array([key], np.uint64))
        return self._get(int(self._segments(h)[0]), int(h[0]), int(key))

    def mixed(self, ops, keys, vals):
        """The batch applied in order -> (values, statuses), as Mixed returns them."""
        keys = np.ascontiguousarray(keys, np.uint64)
        h = hash64(keys)
        seg = self._segments(h).tolist()
        out = np.zeros(keys.size, np.uint64)
        st = np.zeros(keys.size, np.uint8)
        kl, hl, vl = keys.tolist(), h.tolist(), np.asarray(vals, np.uint64).tolist()
        for i, op in enumerate(np.asarray(ops).tolist()):
            if op == OP_INSERT:
                st[i] = self._insert(seg[i], hl[i], kl[i], vl[i])
            else:
                out[i], st[i] = self._get(seg[i], hl[i], kl[i])
        return out, st

    def insert_batch(self, keys, vals):
        return self.mixed(np.ones(len(keys), np.uint8), keys, vals)[1]

    def image(self) -> dict:
        return {"depth": self.depth, "local_depth": self.local_depth.copy(), "prefix": self.prefix.copy(),
                "keys": np.array(self._k, np.uint64).reshape(-1), "values": np.array(self._v, np.uint64).reshape(-1)}


def same_image(a, b) -> bool:
    """Two dump() dicts hold the same table."""
    return (int(a["depth"]) == int(b["depth"])
            and all(np.array_equal(np.asarray(a[f], np.uint64), np.asarray(b[f], np.uint64))
                    for f in ("local_depth", "prefix", "keys", "values")))


def check_table(dump, stats, max_segments):
    """The structure of a valid table, asserted on a dump() dict and the
    engine's stats() (or any dict with "segments")."""
    ld = np.asarray(dump["local_depth"], np.int64)
    n = ld.size
    assert n == stats["segments"], (n, stats["segments"])
    assert n <= max_segments, (n, max_segments)
    # the prefixes tile the hash space: total weight 1, no overlap
    assert np.sum(2.0 ** -ld.astype(np.float64)) == 1.0
    assert np.all(ld <= dump["depth"])
    starts = _starts(ld, dump["prefix"])
    width = np.where(ld == 0, np.float64(2.0 ** 64), 2.0 ** (64 - ld).astype(np.float64))
    assert np.all(np.asarray(dump["prefix"], np.uint64) < (np.uint64(1) << ld.astype(np.uint64)))
    order = np.argsort(starts, kind="stable")
    s = starts[order].astype(np.float64)  # (exact: a start has at most 30 significant bits)
    assert np.all(s[:-1] + width[order][:-1] <= s[1:]), "prefixes overlap"
    keys = np.asarray(dump["keys"], np.uint64).reshape(n, SLOTS)
    vals = np.asarray(dump["values"], np.uint64).reshape(n, SLOTS)
    occ = keys != np.uint64(INVALID)
    assert not np.any(keys == np.uint64(SENTINEL)), "a reserved key is stored"
    assert np.all(vals[~occ] == 0), "an empty slot holds a value"
    si, sl = np.nonzero(occ)
    h = hash64(keys[si, sl])
    ldk = ld[si].astype(np.uint64)
    top = np.where(ldk == 0, np.uint64(0), h >> (np.uint64(64) - np.maximum(ldk, np.uint64(1))))
    assert np.array_equal(top, np.asarray(dump["prefix"], np.uint64)[si]), "a key outside its segment's prefix"
    home = (h & np.uint64(0xFF)).astype(np.int64) * 4
    dist = (sl - home) % SLOTS
    assert np.all(dist < WINDOW), "a key outside its window"
    # no empty slot from the home slot up to the key: empties[a, b) over the row laid out twice
    ce = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(~np.concatenate([occ, occ], axis=1), axis=1)], axis=1)
    assert np.all(ce[si, home + dist] - ce[si, home] == 0), "an empty slot before a stored key in its window"


def stored_pairs(keys, vals, statuses):
    """The (keys, values) of the Inserts answered INSERTED or UPDATED, in order."""
    st = np.asarray(statuses)
    ok = (st == ST_INSERTED) | (st == ST_UPDATED)
    return np.asarray(keys, np.uint64)[ok], np.asarray(vals, np.uint64)[ok]


def check_accounting(dump, inserted_pairs, upsert=False):
    """The stored (key, value) multiset is exactly inserted_pairs: the (keys,
    values) of every op answered INSERTED since the table was empty, in stream
    order; under upsert, of every op answered INSERTED or UPDATED, of which
    each key's last one counts.  Valid while no split dropped an entry."""
    keys, vals = (np.asarray(x, np.uint64) for x in inserted_pairs)
    dk = np.asarray(dump["keys"], np.uint64)
    live = dk != np.uint64(INVALID)
    got = np.stack([dk[live], np.asarray(dump["values"], np.uint64)[live]], axis=1)
    if upsert:
        k, v = keys[::-1], vals[::-1]
        _, first = np.unique(k, return_index=True)  # (of the reversed stream: each key's last write)
        want = np.stack([k[first], v[first]], axis=1)
    else:
        want = np.stack([keys, vals], axis=1)
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    want = want[np.lexsort((want[:, 1], want[:, 0]))]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), "stored pairs differ from the pairs answered INSERTED"
