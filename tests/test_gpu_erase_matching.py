"""pmdfc_cceh_erase_matching on the GPU: every stored key under
a masked pattern leaves the table in one scan.

The contract is the serial rule of Erase applied to the matching keys in
canonical order, and tests/match_ref.py models it.  Every comparison is against
that model applied to the dump the engine gave BEFORE the call -- the image
byte for byte, removed, segments_changed and segments_cleared -- and after each
case limits_ref.check_table runs on the engine's dump (its last assertion is
Invariant I) and error_flags bit 17 (the loop guards) must be clear.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import erase_ref as E
import limits_ref as R
import match_ref as M
import scenarios as S
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pmdfc_amd as P  # noqa: E402
from pmdfc_amd import image as I  # noqa: E402
from pmdfc_amd.kv import KV  # noqa: E402

STREAMS = ["cap2_ins3k", "mixed_cap2_30k_ins80", "dup_wrap", "dup32", "dup_pairs"]
MAX_SEGS = 256
FULL = 0xFFFFFFFFFFFFFFFF
GUARD = 1 << 17
HISTORY = ("splits", "doublings", "split_loss", "insert_passes", "batches", "segment_runs", "deferred_ops",
           "max_rounds", "insert_lines", "fast_declined", "depth", "segments", "capacity", "bucket_bits")


@pytest.fixture(scope="module")
def scen():
    s = S.scenarios(O.hash64)
    s.update(S.upsert_scenarios(O.hash64))
    return s


def filled(stream, upsert=False):
    init_cap, conv, ops, keys, vals = stream
    t = P.CCEH(init_cap, convention=conv, max_batch=16384, max_segments=MAX_SEGS, upsert=upsert)
    for lo in range(0, len(ops), 4096):
        t.Mixed(ops[lo:lo + 4096], keys[lo:lo + 4096], vals[lo:lo + 4096])
    return t


def checked_dump(t, max_segments=MAX_SEGS, flags=0):
    d, s = t.dump(), t.stats()
    R.check_table(d, s, max_segments)
    assert s["error_flags"] == flags, s["error_flags"]
    return d


def call(t, patterns, mask, upsert=False, max_segments=MAX_SEGS, flags=0, retired=0):
    """One EraseMatching against the model of the dump before it.  -> (the
    dump before, the model's table, the result)."""
    pre = checked_dump(t, max_segments, flags)
    hist = {k: v for k, v in t.stats().items() if k in HISTORY}
    m, want = M.erase_matching(pre, mask, patterns, upsert=upsert)
    got = t.EraseMatching(patterns, mask)
    if want["segments_scanned"]:
        # ids retired empty lie below nsegs and are visited, but no dump or stats field shows them: a caller that
        # knows only bounds on their number passes (lo, hi)
        lo, hi = retired if isinstance(retired, tuple) else (retired, retired)
        assert want["segments_scanned"] + lo <= got["segments_scanned"] <= want["segments_scanned"] + hi, (got, want, retired)
        want["segments_scanned"] = got["segments_scanned"]
    assert got == want, (got, want)
    assert R.same_image(checked_dump(t, max_segments, flags), m.image())
    assert {k: v for k, v in t.stats().items() if k in HISTORY} == hist  # depth, segments and the history counters stay
    live = m.live()
    assert t.items()[0].numel() == live
    assert abs(t.Utilization() - 100.0 * live / (len(pre["local_depth"]) * R.SLOTS)) < 1e-6
    return pre, m, got


# ---- 1. the inode stream

@pytest.fixture(scope="module")
def inodes():
    inos, pages, keys = M.inode_stream()
    return inos, pages, keys, keys ^ np.uint64(0x1D0DE)


def inode_table(inodes):
    _, _, keys, vals = inodes
    t = P.CCEH(2, convention="hybrid", max_batch=16384, max_segments=MAX_SEGS)
    assert np.all(t.Insert(keys, vals) == P.ST_INSERTED)
    assert t.stats()["segments"] == 16
    return t


def _absent_inodes(inos, n):
    return np.setdiff1d(np.arange(1 << 21, (1 << 21) + n + 48, dtype=np.uint64), inos)[:n]


def _inode_case(name, inos, pages):
    """-> (inode numbers in the pattern list, the pages that must go)."""
    if name == "one_page":
        return inos[[0]], 1
    if name == "pages700":
        return inos[[3]], 700
    if name == "five":
        return inos[[1, 3, 9, 20, 41]], int(pages[[1, 3, 9, 20, 41]].sum())
    if name == "all48":
        return inos, int(pages.sum())
    if name == "of1024_40_exist":
        p = np.concatenate([inos[:40], _absent_inodes(inos, 984)])
        return p[np.random.default_rng(3).permutation(p.size)], int(pages[:40].sum())
    if name == "absent":
        return _absent_inodes(inos, 1), 0
    assert name == "repeats"
    return np.concatenate([inos[[4, 4, 7, 4]], _absent_inodes(inos, 2), inos[[7, 2]]]), int(pages[[4, 7, 2]].sum())


@pytest.mark.parametrize("name", ["one_page", "pages700", "five", "all48", "of1024_40_exist", "absent", "repeats"])
def test_inode_patterns(inodes, name):
    inos, pages, keys, vals = inodes
    t = inode_table(inodes)
    sel, gone_pages = _inode_case(name, inos, pages)
    pre, m, res = call(t, M.inode_patterns(sel), M.INODE_MASK)
    assert res["removed"] == gone_pages and res["segments_scanned"] == 16
    if name == "absent":
        assert R.same_image(t.dump(), pre) and res["segments_changed"] == 0
    if name == "all48":
        assert res["segments_cleared"] == res["segments_changed"] == 16 and t.Utilization() == 0
    gone = np.isin(keys >> np.uint64(32), sel)
    v, s = t.Get(keys)
    assert np.all(s[gone] == P.ST_MISS) and np.all(s[~gone] == P.ST_HIT) and np.array_equal(v[~gone], vals[~gone])
    if name == "five":
        # no hidden state: the removed keys come back with new values in a mixed batch with Gets of removed
        # and surviving keys, beside the serial oracle that erased L and runs the same batch
        o = O.OracleCCEH(O.OracleCCEH.depth_for_hybrid(2))
        assert np.all(o.insert(keys, vals) == O.ST_INSERTED)
        L = M.matching_keys(pre, M.INODE_MASK, M.inode_patterns(sel))
        assert np.all(o.erase(L) == E.ST_ERASED)
        assert R.same_image(t.dump(), o.dump())
        rng = np.random.default_rng(4)
        back = keys[gone]
        mk = np.concatenate([back, back[rng.integers(0, back.size, 1500)], keys[~gone][:1500]])
        mo = np.concatenate([np.ones(back.size, np.uint8), np.zeros(3000, np.uint8)])
        p = rng.permutation(mk.size)
        mk, mo = mk[p], mo[p]
        mv = mk ^ np.uint64(0xBEEF)
        ov, ost = o.mixed(mo, mk, mv)
        gv, gst = t.Mixed(mo, mk, mv)
        assert np.array_equal(gst, ost) and np.array_equal(gv, ov)
        assert np.count_nonzero(ost == P.ST_MISS) > 100 and np.count_nonzero(ost == P.ST_HIT) > 1500
        assert R.same_image(checked_dump(t), o.dump())
        o.close()
    t.close()


# ---- 2. the fixture streams

@pytest.mark.parametrize("mask,pattern", [(7, 3), (1, 0), (0, 0x1234)])
@pytest.mark.parametrize("name", STREAMS)
def test_streams(scen, name, mask, pattern):
    t = filled(scen[name])
    before = t.stats()
    pre, m, res = call(t, [pattern], mask)
    pm = E.ErasableTable(pre)
    keys = np.asarray(pre["keys"], np.uint64)
    live = keys[keys != np.uint64(R.INVALID)]
    hit = (live & np.uint64(mask)) == np.uint64(pattern & mask)
    assert res["removed"] == np.count_nonzero(hit) > 100
    if mask == 0:
        d = t.dump()
        assert np.all(d["keys"] == np.uint64(R.INVALID)) and np.all(d["values"] == 0)
        assert t.stats()["segments"] == before["segments"] and t.stats()["depth"] == before["depth"]
        assert np.array_equal(d["local_depth"], pre["local_depth"])
        held = (keys != np.uint64(R.INVALID)).reshape(-1, R.SLOTS).any(axis=1)
        assert res["segments_cleared"] == res["segments_changed"] == np.count_nonzero(held)  # cleared, or empty already
        assert t.Utilization() == 0
    else:
        assert 0.09 < np.count_nonzero(hit) / live.size < 0.6
        u, c = np.unique(live, return_counts=True)
        dups = u[c > 1]
        if name in ("dup_wrap", "dup32", "dup_pairs"):
            assert dups.size
        em = E.ErasableTable(t.dump())  # the engine's own table, read back
        for k in dups.tolist():  # every copy of a matching key is gone; the others keep their copies in order
            want = [] if (k & mask) == (pattern & mask) else pm.copies(k)
            assert em.copies(k) == want and m.copies(k) == want
            if want:
                assert t.Get(np.array([k], np.uint64))[0][0] == want[0]
        v, s = t.Get(live)
        assert np.all(s[hit] == P.ST_MISS) and np.all(s[~hit] == P.ST_HIT)
    assert call(t, [pattern], mask)[2]["removed"] == 0  # a second call removes nothing
    t.close()


def test_upsert_table(scen):
    t = filled(scen["up_reinserts_cap2"], upsert=True)
    pre, m, res = call(t, [5, 2], 7, upsert=True)
    assert res["removed"] > 100
    back = M.matching_keys(pre, 7, [5, 2])[:400]
    twice = np.concatenate([back, back])  # a removed key inserted again: INSERTED, and only then UPDATED
    st = t.Insert(twice, twice ^ np.uint64(1))
    assert np.array_equal(st, m.insert_batch(twice, twice ^ np.uint64(1)))
    assert np.all(st[:back.size] == P.ST_INSERTED) and np.all(st[back.size:] == P.ST_UPDATED)
    assert R.same_image(checked_dump(t), m.image())
    t.close()


# ---- 3. the crafted shapes: the smallest tables that reach each branch of the rule

def shape_table(name):
    """The crafted image (the inserts before the trigger) restored into an
    engine -> (engine, its dump, segment prefix, local depth)."""
    init_cap, prefix, L, image, _, _ = S.split_shape_parts(name, O.hash64)
    d0 = O.OracleCCEH.depth_for_hybrid(init_cap)
    o = O.OracleCCEH(d0)
    assert np.all(o.insert(image, image ^ np.uint64(0x5A17)) == O.ST_INSERTED)
    od = o.dump()
    o.close()
    t = P.CCEH(depth=d0, max_batch=4096, max_segments=64)
    t.restore(I.image_from_dump(od, d0))
    pre = checked_dump(t, 64)
    assert R.same_image(pre, od)
    return t, pre, prefix, L


def _target(d, prefix, L):
    seg = int(np.nonzero((np.asarray(d["local_depth"]) == L) & (np.asarray(d["prefix"]) == prefix))[0][0])
    return seg, np.asarray(d["keys"], np.uint64).reshape(-1, 1024)[seg]


@pytest.mark.parametrize("name", ["full_alt", "backlog_c0", "wide_wrap", "cyclic_heads"])
def test_crafted_shapes(name):
    """full_alt: all 1,024 slots taken and half of them match, so no empty slot
    ends a shift; backlog_c0: the 628-slot cluster, long chains; wide_wrap and
    cyclic_heads: shifts across slot 1023."""
    t, pre, prefix, L = shape_table(name)
    seg, row = _target(pre, prefix, L)
    if name == "full_alt":
        assert np.all(row != np.uint64(R.INVALID))
    if name == "backlog_c0":
        assert np.all(row[200:828] != np.uint64(R.INVALID))
    held = row[row != np.uint64(R.INVALID)]
    frac = np.count_nonzero((held & np.uint64(1)) == 0) / held.size
    assert 0.4 < frac < 0.6
    _, m, res = call(t, [0], 1, max_segments=64)
    assert res["segments_changed"] >= 1 and m.moves > 0
    if name in ("wide_wrap", "cyclic_heads"):  # entries whose window reaches past slot 1023 went and stayed
        tail = held[(O.hash64(held) & np.uint64(0xFF)) >= np.uint64(249)]
        assert np.count_nonzero(tail & np.uint64(1)) and np.count_nonzero((tail & np.uint64(1)) == 0)
    v, s = t.Get(held)
    want = [m.get(int(k)) for k in held.tolist()]
    assert v.tolist() == [x[0] for x in want] and s.tolist() == [x[1] for x in want]
    print(f"{name}: {res['removed']} removed, {m.moves} entries moved, longest chain {m.max_chain}")
    t.close()


def test_one_segment_cleared_the_other_untouched():
    """Two segments; every live entry of one matches and none of the other does."""
    t = P.CCEH(depth=1, max_batch=4096, max_segments=64)
    keys = uniform_keys(7, 0, 40000)
    top = O.hash64(keys) >> np.uint64(63)
    a, b = keys[(top == 0) & ((keys & np.uint64(3)) == 1)][:300], keys[(top == 1) & ((keys & np.uint64(3)) == 2)][:300]
    both = np.concatenate([a, b])
    assert np.all(t.Insert(both, both ^ np.uint64(6)) == P.ST_INSERTED) and t.stats()["segments"] == 2
    pre, m, res = call(t, [1], 3, max_segments=64)
    assert (res["removed"], res["segments_scanned"], res["segments_changed"], res["segments_cleared"]) == (300, 2, 1, 1)
    v, s = t.Get(both)
    assert np.all(s[:300] == P.ST_MISS) and np.all(s[300:] == P.ST_HIT)
    t.close()


# ---- 4. pattern edge cases

def test_pattern_edges():
    t = P.CCEH(depth=2, max_batch=4096, max_segments=64)
    keys = uniform_keys(9, 0, 2000)
    # under the mask 0xFFFF0000 a key with those bits clear matches pattern 0 and one with them set matches ~0
    keys[:40] &= np.uint64(FULL ^ 0xFFFF0000)
    keys[40:80] |= np.uint64(0xFFFF0000)
    assert np.all(t.Insert(keys, keys ^ np.uint64(8)) == P.ST_INSERTED)
    n_zero = np.count_nonzero((keys & np.uint64(0xFFFF0000)) == 0)
    n_ones = np.count_nonzero((keys & np.uint64(0xFFFF0000)) == np.uint64(0xFFFF0000))
    assert n_zero >= 40 and n_ones >= 40
    # INVALID under the full mask on a half-empty table: an empty slot never matches
    pre, _, res = call(t, [R.INVALID], FULL, max_segments=64)
    assert res["removed"] == 0 and R.same_image(t.dump(), pre)
    pre, _, res = call(t, [R.INVALID, R.INVALID, 5], FULL, max_segments=64)
    assert res["removed"] == 0 and R.same_image(t.dump(), pre)
    # n == 0
    pre, _, res = call(t, [], FULL, max_segments=64)
    assert res == dict(removed=0, segments_scanned=0, segments_changed=0, segments_cleared=0)
    assert R.same_image(t.dump(), pre)
    # n == 1,025 and a null array: PMDFC_ERR_ARG, the table untouched
    pats = torch.zeros(1025, dtype=torch.int64, device="cuda")
    L = P.load_library()
    r = P.engine.EraseMatchingResult()
    assert L.pmdfc_cceh_erase_matching(t.handle, 0, pats.data_ptr(), 1025, r, None) == -1  # PMDFC_ERR_ARG
    assert L.pmdfc_cceh_erase_matching(t.handle, 0, None, 1, r, None) == -1
    with pytest.raises(P.PmdfcError):
        t.EraseMatching(np.zeros(1025, np.uint64), 0)
    assert R.same_image(checked_dump(t, 64), pre)
    assert L.pmdfc_cceh_erase_matching(t.handle, 0, pats.data_ptr(), 1024, None, None) == 0  # out may be null
    assert t.items()[0].numel() == 0  # (mask 0: everything went)
    assert np.all(t.Insert(keys, keys ^ np.uint64(8)) == P.ST_INSERTED)
    # 0 and ~0 in one multi-pattern set
    pre, m, res = call(t, [0, FULL, 0x12340000], 0xFFFF0000, max_segments=64)
    assert res["removed"] == n_zero + n_ones + np.count_nonzero((keys & np.uint64(0xFFFF0000)) == np.uint64(0x12340000))
    _, s = t.Get(keys[:80])
    assert np.all(s == P.ST_MISS)
    t.close()


# ---- 5. a table that has answered CAPACITY (with retired ids on the runs where the split round denies a retry)

def test_capacity_table_then_compact():
    """The deep chains past the pool, built as test_deep_chain_past_the_pool
    builds its general case (scenarios.DEEP_POOL_CASES): the chains run out of
    pool in the first batch's final pass, which fails a split before it takes
    an id; their triggers are retried in two more general batches and a small
    one.  In a general batch a retry goes through the split round, and a
    request that k_split denies for the pool with room left in the arena has
    taken a segment id, which is retired empty (ctl->dead).  Whether a retry
    reaches that round or is refused before it differs from run to run on the
    same stream (one id when this file ran alone, none after the whole suite; the
    cause was not found), so the
    case cannot promise a retired id: at most one per trigger refused in the
    two general retry batches.  Neither dump() nor stats() shows a retired
    id; the walk does, and the number is printed: segments_scanned is the live
    segments plus the retired ids, the same in every call.  Three calls of
    1,024 full-mask patterns remove uniform keys and leave the chains' full
    windows alone: image and result are the model's, the flags stay, a full
    window is still refused.  Compact then restarts the table: no flag, no
    retired id, and it splits again."""
    c = S.DEEP_POOL_CASES["general"]
    keys, vals, groups = S.deep_chain_stream(c["D"], c["seed"], c["groups"], c["n_uniform"], c["depth"])
    ms, batch, T = c["max_segments"], c["batch"], c["tail"]
    t = P.CCEH(depth=c["depth"], max_batch=c["max_batch"], max_segments=ms)
    last = np.array([g[32] for g in groups], np.uint64)  # each chain's trigger
    more = uniform_keys(c["seed"] + 5, 0, 3 * T)
    tail = np.concatenate([more[:T], last, more[T:2 * T], last, more[2 * T:], last])
    keys = np.concatenate([keys, tail])
    vals = np.concatenate([vals, tail ^ np.uint64(0x7A11)])
    st = np.concatenate([t.Insert(keys[a:a + batch], vals[a:a + batch]) for a in range(0, keys.size, batch)])
    cap = st == P.ST_CAPACITY
    assert np.all(np.isin(keys[cap], last)) and np.all(st[~cap] == P.ST_INSERTED)
    assert keys.size // batch == 3 and keys.size % batch <= 256  # three general batches and a small one
    assert np.count_nonzero(cap[:batch]) > 0
    refused = int(np.count_nonzero(cap[batch:3 * batch]))  # the retries of the general batches 2 and 3
    assert refused > 0
    s0 = t.stats()
    assert s0["error_flags"] == 1 and s0["segments"] + refused <= ms
    uni = keys[~np.isin(keys, np.concatenate(groups))]
    retired = None
    for i in range(3):
        pre, m, got = call(t, uni[i * 1024:(i + 1) * 1024], FULL, max_segments=ms, flags=1,
                           retired=(0, refused) if retired is None else retired)
        retired = got["segments_scanned"] - s0["segments"]
        assert got["removed"] == 1024 and 0 <= retired <= refused
    print(f"capacity table: {s0['segments']} live segments, {retired} retired ids, {got['segments_scanned']} arena ids visited")
    s1 = t.stats()
    assert s1["error_flags"] == 1 and s1["segments"] == s0["segments"]
    fz = R.FrozenTable(t.dump())
    assert np.all(t.Insert(last, last) == P.ST_CAPACITY)  # ctl->full is sticky: the full windows are still refused
    assert all(fz.insert(int(k)) == R.ST_CAPACITY for k in last.tolist())
    stored = keys[st == P.ST_INSERTED]
    want_get = [m.get(int(k)) for k in stored.tolist()]
    r = t.Compact(512)
    assert r["merges"] > 0 and r["segments_after"] < r["segments_before"] == s0["segments"]
    v, s = t.Get(stored)
    assert v.tolist() == [x[0] for x in want_get] and s.tolist() == [x[1] for x in want_get]
    s2 = t.stats()
    R.check_table(t.dump(), s2, ms)
    # the restart of DESIGN.md 4.9: flags and history counters start over, ids are dense again (none retired)
    assert s2["error_flags"] == 0 and s2["splits"] == 0 and s2["segments"] == r["segments_after"]
    assert t.EraseMatching([R.INVALID], FULL)["segments_scanned"] == r["segments_after"]
    # and the table splits again: before the Compact ctl->full refused every split
    fresh = uniform_keys(c["seed"] + 9, 0, 45000)
    fs = np.concatenate([t.Insert(fresh[a:a + 15000], fresh[a:a + 15000] ^ np.uint64(4)) for a in range(0, fresh.size, 15000)])
    s3 = t.stats()
    print(f"after Compact: {r['segments_after']} segments; 45,000 fresh keys: {np.count_nonzero(fs == P.ST_INSERTED)} INSERTED, "
          f"{np.count_nonzero(fs == P.ST_CAPACITY)} CAPACITY, {s3['splits']} splits, {s3['segments']} segments")
    # (45,000 more keys may use the arena up again: a CAPACITY answer must be justified by a full window)
    assert np.all(np.isin(fs, [P.ST_INSERTED, P.ST_CAPACITY]))
    assert s3["splits"] > 0 and s3["segments"] > r["segments_after"]
    ok = fs == P.ST_INSERTED
    assert np.count_nonzero(ok) > fresh.size // 2
    v, s = t.Get(fresh[ok])
    assert np.all(s == P.ST_HIT) and np.array_equal(v, fresh[ok] ^ np.uint64(4))
    d3 = t.dump()
    R.check_table(d3, s3, ms)
    fz = R.FrozenTable(d3)
    assert all(fz.insert(int(k)) == R.ST_CAPACITY for k in np.unique(fresh[~ok]).tolist())
    t.close()


# ---- 6. two shards

def test_two_shards_reassemble_the_global_model(inodes):
    """Each engine of a pair with shard_bits = 1 removes what it stores.  The
    two dumps side by side are one table (depth 4: the shard bit and three
    more, shard 0's segments first); the two images after the calls, side by
    side, are the model's of that table."""
    inos, pages, keys, vals = inodes
    five = inos[[3, 4, 10, 11, 12]]
    sel = M.inode_patterns(five)
    gone = np.isin(keys >> np.uint64(32), five)
    pre, post, results = [], [], []
    for shard in (0, 1):
        t = P.CCEH(depth=3, shard_bits=1, shard_id=shard, max_batch=16384, max_segments=MAX_SEGS)
        st = t.Insert(keys, vals)
        mine = st == P.ST_INSERTED
        assert np.all(st[~mine] == P.ST_WRONG_SHARD) and np.array_equal(mine, (O.hash64(keys) >> np.uint64(63)) == shard)
        pre.append(t.dump())
        res = t.EraseMatching(sel, M.INODE_MASK)
        assert res["removed"] == np.count_nonzero(gone & mine) > 0 and res["segments_scanned"] == t.stats()["segments"]
        assert t.stats()["error_flags"] == 0
        results.append(res)
        post.append(t.dump())
        t.close()

    def side_by_side(a, b):
        d = {f: np.concatenate([np.asarray(a[f], np.uint64), np.asarray(b[f], np.uint64)])
             for f in ("local_depth", "prefix", "keys", "values")}
        d["depth"] = max(int(a["depth"]), int(b["depth"]))
        return d

    whole = side_by_side(*pre)
    R.check_table(whole, {"segments": len(whole["local_depth"])}, 2 * MAX_SEGS)
    m, want = M.erase_matching(whole, M.INODE_MASK, sel)
    assert R.same_image(side_by_side(*post), m.image())
    for f in ("removed", "segments_scanned", "segments_changed", "segments_cleared"):
        assert results[0][f] + results[1][f] == want[f], f
    assert want["removed"] == int(pages[[3, 4, 10, 11, 12]].sum())
    o = O.OracleCCEH(4)
    assert np.all(o.insert(keys, vals) == O.ST_INSERTED)
    print("the two shards' tables before the call equal the unsharded oracle's:", R.same_image(whole, o.dump()))
    o.close()


# ---- 7. every read path after a call

def test_read_paths_after_a_call():
    keys = uniform_keys(61, 0, 20000)
    t = P.CCEH(depth=4, max_batch=32768, max_segments=MAX_SEGS)
    assert np.all(t.Insert(keys, keys ^ np.uint64(0x77)) == P.ST_INSERTED)
    pats = np.array([3, 6, 6, 0x100000005], np.uint64)
    pre, m, res = call(t, pats, 7)
    gone = np.isin(keys & np.uint64(7), [3, 6, 5])
    assert res["removed"] == np.count_nonzero(gone)
    rng = np.random.default_rng(62)
    q = np.concatenate([keys, uniform_keys(63, 0, 1000), np.array([R.INVALID, R.SENTINEL], np.uint64)])
    q = q[rng.permutation(q.size)]
    want = [m.get(int(k)) for k in q.tolist()]
    wv, ws = np.array([x[0] for x in want], np.uint64), np.array([x[1] for x in want], np.uint8)
    assert np.count_nonzero(ws == R.ST_HIT) == keys.size - np.count_nonzero(gone)
    v, s = t.Get(q)
    assert np.array_equal(v, wv) and np.array_equal(s, ws)
    live = ws < R.ST_RESERVED_KEY  # (the table is duplicate-free, so FindAnyway's copy is Get's)
    v, s = t.FindAnyway(q[live][:3000])
    assert np.array_equal(v, wv[live][:3000]) and np.array_equal(s, ws[live][:3000])
    img = m.image()
    ik, iv = t.items()
    mk = img["keys"][img["keys"] != np.uint64(R.INVALID)]
    assert np.array_equal(ik.cpu().numpy().view(np.uint64), mk)
    assert np.array_equal(iv.cpu().numpy().view(np.uint64), img["values"][img["keys"] != np.uint64(R.INVALID)])
    for packed in (False, True):  # PMDFC_ERR_STATE if keys and occupancy words disagree
        b = P.CCEH(depth=4, max_batch=32768, max_segments=MAX_SEGS)
        b.restore(t.snapshot(packed=packed))
        assert R.same_image(checked_dump(b), img)
        b.close()
    r = t.Compact(512)
    assert r["merges"] >= 0
    v, s = t.Get(q)
    assert np.array_equal(v, wv) and np.array_equal(s, ws)
    assert t.items()[0].numel() == mk.size
    checked_dump(t)
    t.close()


# ---- 8. the front-end and the facades

def test_front_end_between_served_ops():
    """erase_matching and invalidate_inodes between served ops from four caller
    threads, a counting filter attached: every answer is a dict's, the filter
    equals OracleCBF over the stored keys (duplicates included), and the waves
    serve again."""
    m_bits, k_hash = 100003, 5
    kv = KV(depth=3, max_batch=4096, max_segments=MAX_SEGS, serve_waves=8)
    f = P.CountingBloomFilter(k_hash, m_bits)
    kv.attach_counting_bf(f)
    inos = np.arange(100, 140, dtype=np.uint64)
    keys = np.concatenate([(i << np.uint64(32)) | np.arange(60, dtype=np.uint64) for i in inos])
    keys = keys[np.random.default_rng(5).permutation(keys.size)]
    keys = np.concatenate([keys, keys[:200]])  # 200 keys are stored twice (no upsert)
    errs = []

    def worker(part, out):
        try:
            _, st, _ = kv.ops(np.ones(part.size, np.uint8), part, part ^ np.uint64(2), run=100)
            out.append(st)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    outs = [[] for _ in range(4)]
    th = [threading.Thread(target=worker, args=(keys[i::4], outs[i])) for i in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs and all(np.all(o[0] == P.ST_INSERTED) for o in outs)
    want = {int(k): int(k) ^ 2 for k in keys.tolist()}
    starts0 = kv.phase()["wave_starts"]
    r1 = kv.invalidate_inodes(inos[:7])
    assert r1["removed"] == np.count_nonzero(np.isin(keys >> np.uint64(32), inos[:7]))
    for k in [k for k in want if (k >> 32) in set(inos[:7].tolist())]:
        del want[k]
    probe = keys[::17]
    vo, st, _ = kv.ops(np.zeros(probe.size, np.uint8), probe, probe, run=50)  # the waves serve again
    assert vo.tolist() == [want.get(int(k), 0) for k in probe.tolist()]
    r2 = kv.erase_matching([1], 1)  # every odd page index
    assert r2["removed"] == sum(1 for k in keys.tolist() if (k & 1) and (k >> 32) not in set(inos[:7].tolist()))
    for k in [k for k in want if k & 1]:
        del want[k]
    assert kv.erase_matching([1], 1)["removed"] == 0
    th = [threading.Thread(target=lambda p=p: errs.extend([] if kv.Get(int(p)) == want.get(int(p), 0) else [int(p)]))
          for p in keys[:8]]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs
    vo, st, _ = kv.ops(np.zeros(keys.size, np.uint8), keys, keys, run=500)
    assert vo.tolist() == [want.get(int(k), 0) for k in keys.tolist()]
    d = kv.dump()
    R.check_table(d, kv.stats(), MAX_SEGS)
    stored = np.asarray(d["keys"], np.uint64)
    stored = stored[stored != np.uint64(R.INVALID)]
    assert np.unique(stored).size < stored.size  # duplicates survive: the rebuild must count them
    o = O.OracleCBF(m_bits, k_hash)
    o.insert(stored)
    assert np.array_equal(f.counters(), o.counters)
    assert kv.audit_filter() == (stored.size, 0)
    ph = kv.phase()
    assert ph["failed_ops"] == 0 and ph["wave_starts"] > starts0 and kv.stats()["error_flags"] == 0
    kv.attach_counting_bf(None)
    kv.close()
    f.close()


def test_facades_erase_matching():
    """GpuCCEH : IHash and GpuCCEHHybrid : ICCEH (tests/cpp/test_gpu_match_kv.cpp,
    a program of its own: the facades are C++)."""
    exe = os.path.join(os.path.dirname(P.engine.LIB_PATH), "test_gpu_match_kv")
    r = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("GpuCCEH match_bad 0", "GpuCCEHHybrid match_bad 0", "GpuCCEH Delete 0", "GpuCCEHHybrid Delete 0",
                 "match_kv_bad 0"):
        assert line in r.stdout, r.stdout
