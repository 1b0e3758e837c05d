"""pmdfc_cceh_compact on the GPU: sibling segments merged to
the fixpoint, their ids back in the arena.

There is no reference implementation of Compact; the contract is the serial
rule, and tests/compact_ref.py models it.  Every comparison here is against
that model applied to the dump the engine gave BEFORE the call, and after each
stream case limits_ref.check_table runs on the engine's dump (its last
assertion is Invariant I).
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import compact_ref as CR
import erase_ref as E
import limits_ref as R
import scenarios as S
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pmdfc_amd as P  # noqa: E402
from pmdfc_amd import image as I  # noqa: E402
from pmdfc_amd.kv import KV  # noqa: E402

STREAMS = ["cap2_ins3k", "mixed_cap2_30k_ins80", "dup_wrap", "dup32", "dup_pairs"]
UPSERT_STREAM = "up_reinserts_cap2"
LIMITS = [256, 512, 1024]
MAX_SEGS = 64
COUNTS = ("segments_before", "segments_after", "merges", "refused", "rounds", "depth_before", "depth_after")


@pytest.fixture(scope="module")
def scen():
    s = S.scenarios(O.hash64)
    s.update(S.upsert_scenarios(O.hash64))
    return s


def checked_dump(t, max_segments=MAX_SEGS):
    d = t.dump()
    s = t.stats()
    R.check_table(d, s, max_segments)
    assert s["error_flags"] == 0
    return d


def erased(stream, upsert=False):
    """The stream filled as tests/test_gpu_erase.py fills it, then its erase
    plan erased -> (engine, the distinct keys that stay)."""
    init_cap, conv, ops, keys, vals = stream
    t = P.CCEH(init_cap, convention=conv, max_batch=16384, max_segments=MAX_SEGS, upsert=upsert)
    for lo in range(0, len(ops), 4096):
        t.Mixed(ops[lo:lo + 4096], keys[lo:lo + 4096], vals[lo:lo + 4096])
    plan, stay = E.erase_plan(keys[np.asarray(ops) == P.OP_INSERT], 77)
    t.Erase(plan)
    return t, stay


_MODELLED = {}


def modelled(case, pre, d0, limit):
    """The model's answer for a case, computed once from the first dump taken
    before a Compact; every later use must start from the same table."""
    if case not in _MODELLED:
        _MODELLED[case] = (pre,) + CR.compact(pre, d0, limit)
    assert R.same_image(pre, _MODELLED[case][0]), "the table before the call differs between cases"
    return _MODELLED[case][1:]


def compact_equals_model(t, case, limit, max_segments=MAX_SEGS, check=True):
    """Compact on engine t against the model of its own dump -> (pre, post, counts)."""
    pre = checked_dump(t, max_segments) if check else t.dump()
    want, res = modelled(case, pre, t.initial_depth, limit)
    got = t.Compact(limit)
    print(f"{case}: {got}")
    assert {k: got[k] for k in COUNTS} == {k: res[k] for k in COUNTS}, (got, res)
    post = checked_dump(t, max_segments) if check else t.dump()
    assert R.same_image(post, want), case
    assert t.stats()["segments"] == res["segments_after"] and t.stats()["depth"] == res["depth_after"]
    if res["merges"]:  # the steps' times: one per round and the round that merged nothing
        tm = t.compact_timing()
        assert len(tm["rounds"]) == res["rounds"] + 1 and tm["gather"] > 0 and tm["restore"] > 0
    return pre, post, res


# ---- 1. the fixture streams

def _stream_case(scen, name, limit, upsert=False):
    t, stay = erased(scen[name], upsert)
    v0, s0 = t.Get(stay)
    assert np.all(s0 == P.ST_HIT)
    n_items = t.items()[0].numel()
    pre, post, res = compact_equals_model(t, (name, limit), limit)
    v1, s1 = t.Get(stay)
    assert np.array_equal(v0, v1) and np.array_equal(s0, s1)
    assert t.items()[0].numel() == n_items == int(np.count_nonzero(np.asarray(pre["keys"]) != np.uint64(R.INVALID)))
    # a second Compact merges nothing and leaves the image identical
    snap = t.snapshot().cpu().numpy().tobytes()
    again = t.Compact(limit)
    assert again["merges"] == 0 and again["rounds"] == 0 and again["segments_after"] == res["segments_after"]
    assert again["refused"] == res["refused"]
    assert t.snapshot().cpu().numpy().tobytes() == snap
    t.close()
    return res


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("name", STREAMS)
def test_stream_compact_equals_model(scen, name, limit):
    _stream_case(scen, name, limit)


def test_upsert_stream_compact_equals_model(scen):
    assert _stream_case(scen, UPSERT_STREAM, 512, upsert=True)["merges"] > 0


def test_arguments():
    t = P.CCEH(depth=2, max_batch=1024, max_segments=16)
    with pytest.raises(P.PmdfcError):
        t.Compact(1025)
    r = t.Compact(0)  # 0 means 512; a fresh table has no segment above the initial depth
    assert r["merges"] == 0 and r["segments_after"] == 4 and r["depth_after"] == 2
    t.close()


# ---- 2. crafted images

def craft(lds, d0, entries, shard_bits=0, shard_id=0):
    """A dump() dict of segments with local depths `lds` (canonical order).
    entries: (segment index, line, count, first) -- `count` keys of that
    segment's prefix and home line, numbered from `first`, placed first-free
    in the order given; values key ^ 0xC0."""
    lds = np.asarray(lds, np.int64)
    span = np.int64(1) << (30 - lds)
    start = np.cumsum(span) - span
    assert int(span.sum()) == 1 << (30 - shard_bits)
    prefix = (np.uint64(shard_id) << (lds - shard_bits).astype(np.uint64)) | (start >> (30 - lds)).astype(np.uint64)
    n = lds.size
    keys = np.full((n, R.SLOTS), R.INVALID, np.uint64)
    vals = np.zeros((n, R.SLOTS), np.uint64)
    placed = []
    for seg, line, count, first in entries:
        ks = S.keys_from_hash_fields(int(prefix[seg]), int(lds[seg]), line, count, first=first)
        for k in ks.tolist():
            free = [j % R.SLOTS for j in range(line * 4, line * 4 + R.WINDOW) if keys[seg, j % R.SLOTS] == np.uint64(R.INVALID)]
            keys[seg, free[0]], vals[seg, free[0]] = k, k ^ 0xC0
            placed.append(k)
    return {"depth": max(d0, int(lds.max())), "local_depth": lds.astype(np.uint32), "prefix": prefix,
            "keys": keys.reshape(-1), "values": vals.reshape(-1)}, np.array(placed, np.uint64)


def restored(d, d0, shard_bits=0, shard_id=0, max_segments=MAX_SEGS):
    t = P.CCEH(depth=d0, shard_bits=shard_bits, shard_id=shard_id, max_batch=4096, max_segments=max_segments)
    t.restore(I.image_from_dump(d, d0, shard_bits, shard_id))
    return t


def _rows(d):
    return np.asarray(d["keys"], np.uint64).reshape(-1, R.SLOTS)


def test_pair_refused_for_a_drop_leaves_the_table_untouched():
    """Child 0 and child 1 hold 20 entries of window 7 each: the 13th entry of
    child 1 finds the window full, at limit 1024.  Nothing merges, so no
    restore runs and the history stays."""
    d, keys = craft([2, 2, 1], 1, [(0, 7, 20, 0), (1, 7, 20, 0), (2, 9, 5, 0)])
    t = restored(d, 1)
    fresh = S.keys_from_hash_fields(1, 1, 200, 3, first=7)
    assert np.all(t.Insert(fresh, fresh) == P.ST_INSERTED)  # (history: a batch has run)
    before, snap = t.stats(), t.snapshot().cpu().numpy().tobytes()
    assert before["batches"] == 1
    pre, post, res = compact_equals_model(t, "refused", 1024)
    assert res["merges"] == 0 and res["refused"] == 1 and res["segments_after"] == 3
    assert t.stats() == before and t.snapshot().cpu().numpy().tobytes() == snap
    # at 20 + 12 the window just fits: merged (the parent is at the initial depth and stays)
    d, keys = craft([2, 2, 1], 1, [(0, 7, 20, 0), (1, 7, 12, 0), (2, 9, 5, 0)])
    t2 = restored(d, 1)
    pre, post, res = compact_equals_model(t2, "fits", 1024)
    assert res["merges"] == 1 and res["rounds"] == 1 and res["refused"] == 0 and post["local_depth"].tolist() == [1, 1]
    assert np.all(_rows(post)[0][28:60] != np.uint64(R.INVALID))
    v, s = t2.Get(keys)
    assert np.all(s == P.ST_HIT) and np.array_equal(v, keys ^ np.uint64(0xC0))
    t.close()
    t2.close()


def test_wrapping_cluster_and_push_past_child0():
    """Child 1's cluster of line 255 wraps past slot 1023 and child 0 holds
    entries of that line too: child 1's follow in their own probe order from
    the cluster's true start.  Child 1's entries of line 10 are pushed past
    child 0's clusters of lines 10 and 11 into line 12."""
    d, keys = craft([2, 2, 1], 1, [(0, 255, 3, 0), (1, 255, 8, 0), (1, 0, 2, 0),
                                  (0, 10, 4, 0), (0, 11, 4, 0), (1, 10, 3, 0), (2, 1, 4, 0)])
    c1 = _rows(d)[1]
    assert np.all(c1[[1020, 1021, 1022, 1023, 0, 1, 2, 3, 4, 5]] != np.uint64(R.INVALID))  # the wrap
    t = restored(d, 1)
    pre, post, res = compact_equals_model(t, "wrap", 1024)
    assert res["merges"] == 1 and post["local_depth"].tolist() == [1, 1]
    p, c0 = _rows(post)[0], _rows(d)[0]
    assert p[1020:1023].tolist() == c0[1020:1023].tolist()
    assert p[[1023, 0, 1, 2, 3, 4, 5, 6]].tolist() == c1[[1020, 1021, 1022, 1023, 0, 1, 2, 3]].tolist()
    assert p[7:9].tolist() == c1[4:6].tolist()  # the line-0 keys behind them
    assert p[40:48].tolist() == c0[40:48].tolist() and p[48:51].tolist() == c1[40:43].tolist()
    v, s = t.Get(keys)
    assert np.all(s == P.ST_HIT) and np.array_equal(v, keys ^ np.uint64(0xC0))
    t.close()


def test_empty_table_collapses_to_the_initial_directory():
    d, _ = craft([4, 4, 3, 5, 5, 4, 3, 3, 3, 3, 3], 3, [])
    t = restored(d, 3)
    pre, post, res = compact_equals_model(t, "empty", 512)
    assert post["local_depth"].tolist() == [3] * 8 and post["depth"] == 3 and res["rounds"] == 2 and res["merges"] == 3
    keys = uniform_keys(7, 0, 3000)
    assert np.all(t.Insert(keys, keys) == P.ST_INSERTED)  # and it grows again
    checked_dump(t)
    t.close()


@pytest.mark.parametrize("shard_id", [0, 1])
def test_sharded_engine(shard_id):
    """shard_bits = 1: the shard's half of the hash space, local depths counted
    in global hash bits, no segment below the initial depth 3."""
    d, keys = craft([4, 4, 3, 5, 5, 4, 3], 3, [(0, 3, 30, 0), (1, 40, 30, 0), (1, 255, 6, 0), (2, 9, 30, 0),
                                              (3, 100, 5, 0), (4, 100, 5, 0), (5, 101, 5, 0), (6, 50, 9, 0)],
                    shard_bits=1, shard_id=shard_id)
    t = restored(d, 3, 1, shard_id)
    assert R.same_image(t.dump(), d)
    pre, post, res = compact_equals_model(t, ("shard", shard_id), 512, check=False)
    assert post["local_depth"].tolist() == [3] * 4 and res["merges"] == 3 and res["rounds"] == 2
    v, s = t.Get(keys)
    assert np.all(s == P.ST_HIT) and np.array_equal(v, keys ^ np.uint64(0xC0))
    assert t.stats()["error_flags"] == 0 and t.items()[0].numel() == keys.size
    t.close()


# ---- 3. no hidden state: the table goes on as the model's image would

def test_continuation_equals_restored_model(scen):
    a, stay = erased(scen["mixed_cap2_30k_ins80"])
    pre = checked_dump(a)
    want, res = CR.compact(pre, a.initial_depth, 1024)
    got = a.Compact(1024)
    assert got["merges"] == res["merges"] > 0 and got["depth_after"] < got["depth_before"]
    b = P.CCEH(depth=a.initial_depth, max_batch=16384, max_segments=MAX_SEGS)
    b.restore(I.image_from_dump(want, a.initial_depth))
    assert a.stats()["bucket_bits"] == b.stats()["bucket_bits"]
    rng = np.random.default_rng(5)
    n = 8192
    ops = (rng.random(n) < 0.6).astype(np.uint8)
    keys = np.where(ops == 1, uniform_keys(55, 0, n), stay[rng.integers(0, stay.size, n)])
    vals = keys ^ np.uint64(0xBEEF)
    for lo in range(0, n, 2048):
        va, sa = a.Mixed(ops[lo:lo + 2048], keys[lo:lo + 2048], vals[lo:lo + 2048])
        vb, sb = b.Mixed(ops[lo:lo + 2048], keys[lo:lo + 2048], vals[lo:lo + 2048])
        assert np.array_equal(sa, sb) and np.array_equal(va, vb), lo
        assert np.all(sa[ops[lo:lo + 2048] == 0] == P.ST_HIT)
    da, db = checked_dump(a), checked_dump(b)
    assert R.same_image(da, db)
    assert a.stats()["splits"] == b.stats()["splits"] > 0 and a.stats()["segments"] > res["segments_after"]
    a.close()
    b.close()


# ---- 4. recovery from CAPACITY

def test_recovery_from_capacity():
    """max_segments = 8, the chain [1,2,3,4,5,6,7,7] nearly empty; one window
    of the depth-1 segment holds 32 distinct keys.  A 33rd key of that window:
    CAPACITY, on a twin without Compact for good.  After Compact the chain is
    [1,1], the same insert is INSERTED and every earlier key still hits."""
    lds = [1, 2, 3, 4, 5, 6, 7, 7]
    d, keys = craft(lds, 1, [(i, 20 + i, 2, 0) for i in range(1, 8)])
    # the 33 keys of window 5 of segment 0 differ right below their prefix: one split separates them
    win = S.keys_from_hash_fields(0, 1, 5, 33, below=(62, 6))
    rows_k, rows_v = _rows(d).copy(), np.asarray(d["values"], np.uint64).reshape(-1, R.SLOTS).copy()
    rows_k[0, 20:52], rows_v[0, 20:52] = win[:32], win[:32] ^ np.uint64(0xC0)
    d["keys"], d["values"] = rows_k.reshape(-1), rows_v.reshape(-1)
    keys = np.concatenate([keys, win[:32]])
    extra = win[32:]
    a, b = restored(d, 1, max_segments=8), restored(d, 1, max_segments=8)
    for t in (a, b):
        assert R.same_image(checked_dump(t, 8), d)
        assert t.Insert(extra, extra).tolist() == [P.ST_CAPACITY]
    pre, post, res = compact_equals_model(a, "chain", 512, max_segments=8)
    assert post["local_depth"].tolist() == [1, 1] and res["merges"] == 6 and res["depth_after"] == 1
    assert a.Insert(extra, extra ^ np.uint64(0xC0)).tolist() == [P.ST_INSERTED]
    assert b.Insert(extra, extra).tolist() == [P.ST_CAPACITY]
    allk = np.concatenate([keys, extra])
    v, s = a.Get(allk)
    assert np.all(s == P.ST_HIT) and np.array_equal(v, allk ^ np.uint64(0xC0))
    assert a.stats()["splits"] >= 1 and a.stats()["segments"] <= 8
    checked_dump(a, 8)
    a.close()
    b.close()


# ---- 5. the front-end

def test_front_end_compact_between_ring_ops():
    """KV.compact while two threads run ring ops: the table before and after
    equal the model, every Get hits, the attached filter stays exact."""
    m_bits, k_hash = 100003, 5
    keys = uniform_keys(81, 0, 6000)
    kv = KV(depth=3, max_batch=2048, max_segments=256, serve_waves=8)
    f = P.CountingBloomFilter(k_hash, m_bits)
    kv.attach_counting_bf(f)
    _, st, _ = kv.ops(np.ones(keys.size, np.uint8), keys, keys ^ np.uint64(2), run=500)
    assert np.all(st == P.ST_INSERTED)
    gone = np.random.default_rng(82).random(keys.size) < 0.75
    assert np.all(kv.erase_run(keys[gone]) == P.ST_ERASED)
    stay = keys[~gone]
    pre = kv.dump()
    R.check_table(pre, kv.stats(), 256)
    want, res = CR.compact(pre, 3, 512)
    assert res["merges"] > 0
    errs, out = [], {}

    def caller(i):
        try:
            for _ in range(3):
                k = stay[i::2]
                vo, s, _ = kv.ops(np.zeros(k.size, np.uint8), k, k, run=100)
                assert np.all(s == P.ST_HIT) and np.array_equal(vo, k ^ np.uint64(2))
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    th = [threading.Thread(target=caller, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    out = kv.compact(512)
    for x in th:
        x.join()
    assert not errs, errs
    assert {k: out[k] for k in COUNTS} == {k: res[k] for k in COUNTS}, (out, res)
    post = kv.dump()
    R.check_table(post, kv.stats(), 256)
    assert R.same_image(post, want)
    assert kv.audit_filter() == (stay.size, 0)
    vo, s, _ = kv.ops(np.zeros(keys.size, np.uint8), keys, keys, run=500)  # the waves serve again
    assert np.all(s[gone] == P.ST_MISS) and np.all(s[~gone] == P.ST_HIT)
    assert kv.compact(512)["merges"] == 0
    assert kv.stats()["error_flags"] == 0 and kv.phase()["failed_ops"] == 0
    kv.attach_counting_bf(None)
    kv.close()
    f.close()


def test_facades_compact():
    """GpuCCEH : IHash and GpuCCEHHybrid : ICCEH (tests/cpp/test_gpu_compact_kv.cpp,
    a program of its own: the facades are C++): Compact after EraseBatch with a
    filter attached, refused from a completion callback."""
    exe = os.path.join(os.path.dirname(P.engine.LIB_PATH), "test_gpu_compact_kv")
    r = subprocess.run([exe, "12000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("GpuCCEH callback_bad 0", "GpuCCEHHybrid callback_bad 0", "GpuCCEH compact_trip_bad 0",
                 "GpuCCEHHybrid compact_trip_bad 0", "compact_kv_bad 0"):
        assert line in r.stdout, r.stdout
    assert " shape_bad 0" in r.stdout, r.stdout
