"""unhash64 and the model of a table that cannot split (tests/limits_ref.py)
against the serial oracle, on the CPU; and the condition every stream of
tests/test_gpu_limits.py rests on: no split of the serial table drops an entry.
"""
import os

import numpy as np
import pytest

import limits_ref as R
import scenarios as S
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys


def test_unhash64_inverts_hash64(golden_dir):
    kat = np.load(os.path.join(golden_dir, "hash_kat.npz"))
    rnd = np.random.default_rng(64).integers(0, 1 << 64, 1 << 16, dtype=np.uint64)
    edge = np.array([0, 1, 2**64 - 1, 2**64 - 2, 1 << 63, 0xc70697], np.uint64)
    for x in (kat["keys"], kat["h"], rnd, edge):
        assert np.array_equal(O.hash64(S.unhash64(x)), x)
        assert np.array_equal(S.unhash64(O.hash64(x)), x)
    assert np.array_equal(S.unhash64(kat["h"]), kat["keys"])
    # the numpy hash of the model is the oracle's
    assert np.array_equal(R.hash64(kat["keys"]), kat["h"]) and np.array_equal(R.hash64(rnd), O.hash64(rnd))


def test_keys_from_hash_fields():
    k = S.keys_from_hash_fields(0x2B5, 10, 201, 500, first=3)
    h = O.hash64(k)
    assert np.unique(k).size == 500
    assert np.all(h >> np.uint64(54) == np.uint64(0x2B5)) and np.all(h & np.uint64(0xFF) == np.uint64(201))
    assert np.array_equal((h >> np.uint64(8)) & np.uint64((1 << 46) - 1), np.arange(3, 503, dtype=np.uint64))
    # numbered right below a 21-bit prefix: bit 42 tells the last key from the first 32
    k = S.keys_from_hash_fields(0x12345, 21, 255, 33, below=(42, 6))
    h = O.hash64(k)
    assert np.all(h >> np.uint64(43) == np.uint64(0x12345)) and np.all(h & np.uint64(0xFF) == np.uint64(255))
    assert np.array_equal((h >> np.uint64(42)) & np.uint64(1), np.arange(33, dtype=np.uint64) >> np.uint64(5))
    assert np.unique(k).size == 33
    assert S.keys_from_hash_fields(0, 0, 9, 4).size == 4


def _preloaded(upsert):
    o = O.OracleCCEH(8, upsert=upsert)
    pre = uniform_keys(301, 0, 60000)
    assert np.all(o.insert(pre, pre ^ np.uint64(0x51)) == O.ST_INSERTED)
    return o, pre


@pytest.mark.parametrize("upsert", [False, True], ids=["insert", "upsert"])
def test_frozen_table_equals_oracle_while_nothing_splits(upsert):
    """A mixed stream that fills no window (every insert INSERTED / UPDATED,
    the segment count unchanged): FrozenTable is the oracle, op by op and
    slot by slot.  The stream re-inserts stored keys, inserts one fresh key
    twice in a row and asks for stored, fresh and absent keys."""
    o, pre = _preloaded(upsert)
    nseg = o.num_segments
    f = R.FrozenTable(o.dump(), upsert=upsert)
    assert R.same_image(f.image(), o.dump())
    rng = np.random.default_rng(302)
    fresh = uniform_keys(301, 60000, 6000)
    twice = np.repeat(uniform_keys(303, 0, 50), 2)
    ins = np.concatenate([fresh, rng.choice(pre, 1500)])
    gets = np.concatenate([rng.choice(pre, 3000), rng.choice(fresh, 2000), uniform_keys(304, 0, 1000), twice,
                           np.array([2**64 - 1, 2**64 - 2], np.uint64)])
    keys = np.concatenate([ins, gets])
    ops = np.concatenate([np.ones(ins.size, np.uint8), np.zeros(gets.size, np.uint8)])
    p = rng.permutation(keys.size)
    # shuffled, with the batch that inserts each of 50 keys twice in a row in the middle
    keys = np.concatenate([keys[p[:5000]], twice, keys[p[5000:]]])
    ops = np.concatenate([ops[p[:5000]], np.ones(twice.size, np.uint8), ops[p[5000:]]])
    vals = np.where(ops == 1, np.arange(1, keys.size + 1, dtype=np.uint64), np.uint64(0)).astype(np.uint64)
    ov, ost = o.mixed(ops, keys, vals)
    assert o.num_segments == nseg and o.stats()["split_loss"] == 0
    good = (O.ST_INSERTED, O.ST_UPDATED) if upsert else (O.ST_INSERTED,)
    assert np.all(np.isin(ost[ops == 1], good)), "the stream filled a window"
    fv, fst = f.mixed(ops, keys, vals)
    assert np.array_equal(fst, ost) and np.array_equal(fv, ov)
    assert R.same_image(f.image(), o.dump())
    if upsert:
        assert np.count_nonzero(fst == R.ST_UPDATED) >= 1500 + 50
    R.check_table(o.dump(), {"segments": nseg}, nseg)
    ik, iv = R.stored_pairs(np.concatenate([pre, keys[ops == 1]]),
                            np.concatenate([pre ^ np.uint64(0x51), vals[ops == 1]]),
                            np.concatenate([np.full(pre.size, O.ST_INSERTED, np.uint8), ost[ops == 1]]))
    R.check_accounting(o.dump(), (ik, iv), upsert=upsert)
    # one op at a time gives the same answers as the batch
    f2 = R.FrozenTable(o.dump(), upsert=upsert)
    assert f2.get(int(pre[5])) == (int(pre[5] ^ np.uint64(0x51)), R.ST_HIT)
    assert f2.get(12345678901) == (0, R.ST_MISS)


def _hand_table(entries):
    """A depth-1 table of two segments; entries: (key, value) pairs placed as
    Insert would place them."""
    d = {"depth": 1, "local_depth": np.array([1, 1], np.uint32), "prefix": np.array([0, 1], np.uint64),
         "keys": np.full(2048, R.INVALID, np.uint64), "values": np.zeros(2048, np.uint64)}
    f = R.FrozenTable(d)
    for k, v in entries:
        assert f.insert(k, v) == R.ST_INSERTED
    return f


def test_frozen_table_full_window_capacity():
    """32 distinct keys of home line 255 in segment 1 fill the wrapping window
    1020..1023, 0..27: a 33rd answers CAPACITY and changes nothing; its
    neighbours' windows still take keys; a stored key is still a HIT."""
    ks = S.keys_from_hash_fields(1, 1, 255, 34)
    f = _hand_table([(int(k), i + 1) for i, k in enumerate(ks[:32])])
    img = f.image()
    slots = np.nonzero(img["keys"][1024:] != np.uint64(R.INVALID))[0]
    assert slots.tolist() == list(range(28)) + [1020, 1021, 1022, 1023]
    assert np.array_equal(img["keys"][1024 + 1020:2048], ks[:4]) and np.array_equal(img["keys"][1024:1024 + 28], ks[4:32])
    before = f.image()
    assert f.insert(int(ks[32]), 99) == R.ST_CAPACITY and f.insert(int(ks[33]), 99) == R.ST_CAPACITY
    assert R.same_image(f.image(), before)
    assert f.get(int(ks[32])) == (0, R.ST_MISS) and f.get(int(ks[31])) == (32, R.ST_HIT)
    # line 254's window [1016, 1048) has 4 free slots left, line 0's [0, 32) also 4
    for line, room in ((254, 4), (0, 4)):
        kk = S.keys_from_hash_fields(1, 1, line, 5, first=100)
        st = f.insert_batch(kk, kk)
        assert st.tolist() == [R.ST_INSERTED] * room + [R.ST_CAPACITY] * (5 - room)
    # the same hash fields in segment 0 are another window
    assert f.insert(int(S.keys_from_hash_fields(0, 1, 255, 1)[0]), 5) == R.ST_INSERTED
    assert f.insert(2**64 - 1, 5) == R.ST_RESERVED_KEY and f.insert(2**64 - 2, 5) == R.ST_RESERVED_KEY
    R.check_table(f.image(), {"segments": 2}, 2)
    # under upsert a stored key of the full window is still updated in place
    u = R.FrozenTable(before, upsert=True)
    assert u.insert(int(ks[7]), 777) == R.ST_UPDATED and u.get(int(ks[7])) == (777, R.ST_HIT)
    assert u.insert(int(ks[32]), 99) == R.ST_CAPACITY


def test_frozen_table_full_window_unsplittable():
    """32 copies of one key fill its window: the 33rd answers UNSPLITTABLE (no
    split could separate them), another key of that home line CAPACITY."""
    k = int(S.keys_from_hash_fields(0, 1, 100, 1)[0])
    f = _hand_table([(k, i + 1) for i in range(32)])
    before = f.image()
    assert f.insert(k, 33) == R.ST_UNSPLITTABLE
    assert f.insert(int(S.keys_from_hash_fields(0, 1, 100, 1, first=1)[0]), 1) == R.ST_CAPACITY
    assert R.same_image(f.image(), before)
    assert f.get(k) == (1, R.ST_HIT)
    o = O.OracleCCEH(1)
    ost = o.insert(np.full(33, k, np.uint64), np.arange(1, 34, dtype=np.uint64))
    assert ost.tolist() == [O.ST_INSERTED] * 32 + [O.ST_UNSPLITTABLE]
    assert R.same_image(before, o.dump())


def test_check_table_and_accounting_reject_broken_tables():
    o, pre = _preloaded(False)
    d = o.dump()
    n = o.num_segments
    pairs = (pre, pre ^ np.uint64(0x51))
    R.check_table(d, {"segments": n}, n)
    R.check_accounting(d, pairs)

    def broken(**kw):
        b = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in d.items()}
        for name, (i, x) in kw.items():
            b[name][i] = x
        return b
    s0 = int(np.nonzero(d["keys"] != np.uint64(R.INVALID))[0][0])
    e0 = int(np.nonzero(d["keys"] == np.uint64(R.INVALID))[0][0])
    with pytest.raises(AssertionError):
        R.check_table(d, {"segments": n + 1}, n + 1)
    with pytest.raises(AssertionError):
        R.check_table(d, {"segments": n}, n - 1)
    with pytest.raises(AssertionError):  # a key of another segment
        R.check_table(broken(keys=(s0, d["keys"][d["keys"] != np.uint64(R.INVALID)][-1])), {"segments": n}, n)
    with pytest.raises(AssertionError):  # a value in an empty slot
        R.check_table(broken(values=(e0, 7)), {"segments": n}, n)
    with pytest.raises(AssertionError):  # a hole before a stored key: its home slot emptied
        h = R.hash64(d["keys"])
        live = d["keys"] != np.uint64(R.INVALID)
        away = np.nonzero(live & (((np.arange(d["keys"].size) % 1024) - (h & np.uint64(0xFF)).astype(np.int64) * 4) % 1024 > 0))[0]
        i = int(away[0])
        home = i - i % 1024 + int(h[i] & np.uint64(0xFF)) * 4
        R.check_table(broken(keys=(home, R.INVALID), values=(home, 0)), {"segments": n}, n)
    with pytest.raises(AssertionError):  # overlapping prefixes
        R.check_table(broken(prefix=(1, d["prefix"][0])), {"segments": n}, n)
    with pytest.raises(AssertionError):  # a lost pair
        R.check_accounting(broken(keys=(s0, R.INVALID), values=(s0, 0)), pairs)
    with pytest.raises(AssertionError):  # a changed value
        R.check_accounting(broken(values=(s0, 1)), pairs)


def _unlimited_split_loss(depth, keys, vals, upsert=False):
    o = O.OracleCCEH(depth, upsert=upsert)
    o.insert(keys, vals)
    return o.stats()["split_loss"]


def test_limit_streams_drop_nothing():
    """The condition on the inputs of tests/test_gpu_limits.py: on the serial
    table with no segment limit, no split of any stream drops an entry (then
    none does on a table that stops splitting earlier: its splits are the
    first of the same serial run)."""
    seen = set()
    for name, c in S.LIMIT_CASES.items():
        key = (c["seed"], c["depth"], c["extra"], c.get("upsert", False))
        if key in seen:
            continue
        seen.add(key)
        ms = (1 << c["depth"]) + c["extra"]
        if c.get("upsert"):
            keys, vals = S.limit_upsert_stream(c["seed"], ms)
        else:
            keys, vals = S.limit_stream(c["seed"], ms)
        assert _unlimited_split_loss(c["depth"], keys, vals, c.get("upsert", False)) == 0, name
    for D, seed in S.DEEP_CHAIN_CASES:
        keys, vals, groups = S.deep_chain_stream(D, seed)
        o = O.OracleCCEH(S.DEEP_CHAIN_DEPTH)
        st = o.insert(keys, vals)
        assert np.all(st == O.ST_INSERTED) and o.stats()["split_loss"] == 0, (D, seed)
        # the shape the stream is for: a directory of depth D over few segments
        assert o.depth == D and o.num_segments == (1 << S.DEEP_CHAIN_DEPTH) + len(groups) * (D - S.DEEP_CHAIN_DEPTH)
    for name in ("small", "general"):  # ("medium" is the stream of "small")
        c = S.DEEP_POOL_CASES[name]
        keys, vals, groups = S.deep_chain_stream(c["D"], c["seed"], c["groups"], c["n_uniform"], c["depth"])
        assert _unlimited_split_loss(c["depth"], keys, vals) == 0, name
