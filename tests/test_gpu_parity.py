"""Parity of the HIP engine (through the C-ABI) with the reference.

* golden scenarios: fixtures produced by the reference's own CCEH_hybrid.cpp
  (tests/golden/gen_golden.py) -- final directory depth, canonical segment
  images (keys and values, slot for slot), Get results of every op;
* the same scenarios cut into ragged batches, through the Mixed and the
  Insert/Get entry points (batch semantics == serial semantics);
* full-size configs through size-independent properties and the oracle.
Bit-exact throughout (integer path, no tolerance).
"""
import json
import os

import numpy as np
import pytest

import scenarios as S
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pmdfc_amd as P  # noqa: E402

NAMES = ["cap2_ins3k", "cap8_ins20k", "cap1024_ins100k", "cap2_ins100k", "cap256_ins400k",
         "mixed_cap16_60k", "mixed_cap2_30k_ins80", "dup_wrap", "dup32", "dup_pairs",
         "src_cap2m_ins50k"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "cceh_scenarios.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scen():
    return S.scenarios(O.hash64)


def _summary(t, ops, out):
    d = t.dump()
    return S.summarize(d["depth"], d["local_depth"], d["prefix"], d["keys"], d["values"], out, ops)


def _check(rec, g, name):
    for k, v in rec.items():
        assert v == g[k], (name, k, v, g[k])


def test_gpu_hash_kat(golden_dir):
    kat = np.load(os.path.join(golden_dir, "hash_kat.npz"))
    assert np.array_equal(P.hash64(kat["keys"]), kat["h"])


def test_gpu_gen_keys_matches_numpy():
    for seed, start, n in [(0, 0, 1000), (5, 123456, 4097), (3, 1 << 30, 100)]:
        d = P.gen_keys(seed, start, n).cpu().numpy().view(np.uint64)
        assert np.array_equal(d, uniform_keys(seed, start, n))


@pytest.fixture(params=["default", "tight"])
def path(request, monkeypatch):
    """default: the engine's own bucket/chunk geometry; tight: at most 2
    buckets and 61-op chunks, so every scenario crosses many chunk boundaries,
    waits through many split rounds and grows sub-directories by many levels
    inside one bucket (bucket_pass.h); its Gets skip the flattened directory
    beyond 3 bits (the hdr/pool fallback of dir_entry)."""
    if request.param == "tight":
        monkeypatch.setenv("PMDFC_P1MAX", "1")
        monkeypatch.setenv("PMDFC_CHUNK", "61")
        monkeypatch.setenv("PMDFC_FLAT_MAX", "3")
    else:
        monkeypatch.delenv("PMDFC_P1MAX", raising=False)
        monkeypatch.delenv("PMDFC_CHUNK", raising=False)
        monkeypatch.delenv("PMDFC_FLAT_MAX", raising=False)
    return request.param


@pytest.mark.parametrize("batch", [0, 997, 65536])
@pytest.mark.parametrize("name", NAMES)
def test_mixed_matches_reference(name, batch, golden, scen, path):
    init_cap, conv, ops, keys, vals = scen[name]
    n = keys.size
    b = batch or n
    t = P.CCEH(init_cap, convention=conv, max_batch=b, max_segments=8192)
    out = np.zeros(n, np.uint64)
    st = np.zeros(n, np.uint8)
    for off in range(0, n, b):
        o, s = t.Mixed(ops[off:off + b], keys[off:off + b], vals[off:off + b])
        out[off:off + b] = o
        st[off:off + b] = s
    _check(_summary(t, ops, out), golden[name], name)
    g = golden[name]
    if "get_values_sample" in g:
        assert out[g["get_positions_sample"]].tolist() == g["get_values_sample"]
    ins = ops == S.OP_INSERT
    assert np.all(st[ins] == P.ST_INSERTED)
    assert np.all((st[~ins] == P.ST_HIT) == (out[~ins] != 0))
    s = t.stats()
    assert s["split_loss"] == 0
    assert s["error_flags"] == 0  # no device-side assumption tripped
    ou = O.OracleCCEH(t.initial_depth)
    ou.mixed(ops, keys, vals)
    assert abs(t.Utilization() - ou.utilization()) < 1e-9
    assert t.Capacity() == g["capacity"]
    t.close()


@pytest.fixture(scope="module")
def findany_golden(golden_dir):
    with open(os.path.join(golden_dir, "findany.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("batch", [0, 997])
@pytest.mark.parametrize("name", S.FINDANY_CASES)
def test_find_anyway_matches_reference(name, batch, findany_golden, scen):
    """pmdfc_cceh_find_anyway == the reference's CCEH::FindAnyway
    (CCEH_hybrid.cpp:482-496, src/cceh.cpp:457-471) after each stream, key for
    key (tests/golden/findany.json), and == the oracle's literal scan; in
    dup_wrap one key's first copy in slot order is not Get's."""
    g = findany_golden[name]
    init_cap, conv, ops, keys, vals = scen[name]
    n = keys.size
    b = batch or n
    t = P.CCEH(init_cap, convention=conv, max_batch=b, max_segments=8192)
    for off in range(0, n, b):
        t.Mixed(ops[off:off + b], keys[off:off + b], vals[off:off + b])
    q = S.findany_queries(keys)
    fa, fst = t.FindAnyway(q)
    gv, _ = t.Get(q)
    assert S.sha(fa) == g["find_sha"] and S.sha(gv) == g["get_sha"]
    assert np.array_equal(fst == P.ST_HIT, fa != 0)
    div = np.nonzero(fa != gv)[0]
    assert [[int(i), int(fa[i]), int(gv[i])] for i in div] == g["diverge"]
    o = O.OracleCCEH(t.initial_depth)
    o.mixed(ops, keys, vals)
    ofa, ost = o.find_anyway(q)
    assert np.array_equal(fa, ofa) and np.array_equal(fst, ost)
    rv, rst = t.FindAnyway(np.array([2**64 - 1, 2**64 - 2], np.uint64))
    assert rst.tolist() == [P.ST_RESERVED_KEY] * 2 and rv.tolist() == [0, 0]
    t.close()


@pytest.mark.parametrize("name", ["cap2_ins3k", "cap8_ins20k", "cap2_ins100k", "cap256_ins400k",
                                  "cap1024_ins100k", "src_cap2m_ins50k", "dup_pairs"])
def test_insert_get_entry_points(name, golden, scen, path):
    """Pure Insert batches then pure Get batches (the sync-free k_get path)."""
    init_cap, conv, ops, keys, vals = scen[name]
    ins = ops == S.OP_INSERT
    assert ins[: ins.sum()].all()  # inserts first in these scenarios
    t = P.CCEH(init_cap, convention=conv, max_batch=1 << 16, max_segments=8192)
    ik, iv = keys[ins], vals[ins]
    st = t.Insert(ik, iv)
    assert np.all(st == P.ST_INSERTED)
    gk = keys[~ins]
    out, gst = t.Get(gk)
    full = np.zeros(keys.size, np.uint64)
    full[~ins] = out
    _check(_summary(t, ops, full), golden[name], name)
    assert np.all((gst == P.ST_HIT) == (out != 0))
    t.close()


def test_device_tensor_path_async():
    """Zero-copy torch tensors on the current stream."""
    t = P.CCEH(depth=4, max_batch=1 << 14, max_segments=4096)
    k = P.gen_keys(77, 0, 50000)
    v = k ^ 0x5A5A
    st = t.Insert(k, v)
    out, gst = t.Get(k)
    torch.cuda.synchronize()
    assert bool((st == P.ST_INSERTED).all())
    assert bool((gst == P.ST_HIT).all()) and bool((out == v).all())
    t.close()


def test_gets_between_insert_batches_follow_splits():
    """The flattened Get directory is rebuilt after every insert batch: Gets
    interleaved with split-heavy inserts hit every key inserted so far."""
    t = P.CCEH(depth=4, max_batch=1 << 16, max_segments=4096)
    seen = np.zeros(0, np.uint64)
    for r in range(6):
        k = uniform_keys(91, r * 50000, 50000)
        assert np.all(t.Insert(k, k ^ np.uint64(7)) == P.ST_INSERTED)
        seen = np.concatenate([seen, k])
        v, st = t.Get(seen)
        assert np.all(st == P.ST_HIT) and np.array_equal(v, seen ^ np.uint64(7)), r
    miss = uniform_keys(92, 0, 20000)
    assert np.all(t.Get(miss)[1] == P.ST_MISS)
    t.close()


@pytest.mark.parametrize("depth,batch", [(10, 65536), (3, 20000)])
def test_reset_gives_a_fresh_table(depth, batch):
    """pmdfc_cceh_reset (the bench resets every step, with no host sync:
    cceh_engine.hip init_state): after each reset the table is a fresh
    CCEH(initCap).  Rounds of alternating size, so a small round runs over
    segments a bigger round filled: every round's statuses, Gets, canonical
    table, utilization and capacity equal the oracle's over that round's
    stream alone, and the keys of the round before miss."""
    t = P.CCEH(depth=depth, max_batch=batch, max_segments=16384)
    prev = None
    for r in range(5):
        if r:
            t.reset()
        n = 150000 if r % 2 == 0 else 40000
        keys = uniform_keys(200 + r, 0, n)
        vals = keys ^ np.uint64(r + 1)
        o = O.OracleCCEH(t.initial_depth)
        if r % 2:  # a mixed round (the mixed batches' key set must start empty after a reset)
            ops = np.where(np.arange(n) % 3 == 2, S.OP_GET, S.OP_INSERT).astype(np.uint8)
            gk = keys.copy()
            gk[2::3] = keys[np.arange(2, n, 3) // 2]  # Gets of keys inserted earlier in the round
            out, mst = t.MixedBatches(ops, gk, vals, list(range(0, n, batch)) + [n])
            ov, ost = o.mixed(ops, gk, vals)
            assert np.array_equal(mst, ost) and np.array_equal(out, ov), r
            keys, vals = gk[ops == S.OP_INSERT], vals[ops == S.OP_INSERT]
        else:
            st = t.InsertBatches(keys, vals, list(range(0, n, batch)) + [n])
            assert np.array_equal(st, o.insert(keys, vals)), r
        v, gs = t.Get(keys)
        ov, ost = o.get(keys)
        assert np.array_equal(gs, ost) and np.array_equal(v, ov), r
        if prev is not None:
            assert np.all(t.Get(prev)[1] == P.ST_MISS), r
        d, od = t.dump(), o.dump()
        assert d["depth"] == od["depth"], r
        for f in ("local_depth", "keys", "values"):
            assert np.array_equal(d[f], od[f]), (r, f)
        assert abs(t.Utilization() - o.utilization()) < 1e-9, r
        assert t.Capacity() == o.capacity(), r
        assert t.stats()["error_flags"] == 0
        prev = keys
    t.close()


@pytest.mark.parametrize("sizes", [[5000, 1, 0, 7000, 65536, 300, 65536, 12000], [65536] * 6])
def test_insert_batches_equals_batch_by_batch(sizes):
    """pmdfc_cceh_insert_batches (partition of batch i+1 overlapping batch i)
    leaves exactly the table and statuses of one Insert per batch, and the
    one-batch entry points keep working after it."""
    n = sum(sizes)
    keys = uniform_keys(93, 0, n + 4000)
    keys[1000:1040] = keys[1000]  # a duplicate run: UNSPLITTABLE inside a batch
    vals = keys ^ np.uint64(0xABC)
    bounds = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    a = P.CCEH(depth=3, max_batch=1 << 16, max_segments=8192)
    b = P.CCEH(depth=3, max_batch=1 << 16, max_segments=8192)
    sa = np.concatenate([a.Insert(keys[bounds[i]:bounds[i + 1]], vals[bounds[i]:bounds[i + 1]])
                         for i in range(len(sizes))])
    sb = b.InsertBatches(keys[:n], vals[:n], bounds)
    assert np.array_equal(sa, sb)
    for t in (a, b):  # a one-batch call after the pipelined ones
        assert np.all(t.Insert(keys[n:], vals[n:]) == P.ST_INSERTED)
    da, db_ = a.dump(), b.dump()
    for f in ("local_depth", "keys", "values"):
        assert np.array_equal(da[f], db_[f]), f
    v, st = b.Get(keys)
    hit = st == P.ST_HIT
    assert hit.sum() >= n + 4000 - 40 and np.array_equal(v[hit], vals[hit])
    a.close()
    b.close()


@pytest.mark.parametrize("name,batch", [("mixed_cap16_60k", 10000), ("mixed_cap2_30k_ins80", 9000),
                                        ("dup_pairs", 9000), ("cap1024_ins100k", 20000),
                                        ("cap256_ins400k", 65536)])
def test_mixed_batches_match_oracle(name, batch, scen, path):
    """pmdfc_cceh_mixed_batches == the serial oracle, op by op and table by
    table, over ragged batch sequences of the general path (the tight path
    reaches its final bucket resolution at once)."""
    init_cap, conv, ops, keys, vals = scen[name]
    n = keys.size
    bounds = list(range(0, n, batch)) + [n]
    t = P.CCEH(init_cap, convention=conv, max_batch=batch, max_segments=16384)
    out, st = t.MixedBatches(ops, keys, vals, bounds)
    o = O.OracleCCEH(t.initial_depth)
    ov, ost = o.mixed(ops, keys, vals)
    bad = np.nonzero((st != ost) | (out != ov))[0]
    assert bad.size == 0, (name, bad[:8], st[bad[:8]], ost[bad[:8]])
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"]
    for f in ("local_depth", "keys", "values"):
        assert np.array_equal(d[f], od[f]), f
    # a one-batch call after them
    o2, s2 = t.Mixed(ops[:batch], keys[:batch], vals[:batch])
    ov2, ost2 = o.mixed(ops[:batch], keys[:batch], vals[:batch])
    assert np.array_equal(s2, ost2) and np.array_equal(o2, ov2)
    assert t.stats()["error_flags"] == 0
    t.close()


def test_dup33_unsplittable_and_table_unchanged():
    t = P.CCEH(depth=2, max_batch=64, max_segments=64)
    k = np.full(34, 12345, np.uint64)
    st = t.Insert(k, np.arange(1, 35, dtype=np.uint64))
    assert np.all(st[:32] == P.ST_INSERTED) and np.all(st[32:] == P.ST_UNSPLITTABLE)
    v, s = t.Get(np.array([12345], np.uint64))
    assert s[0] == P.ST_HIT and v[0] == 1
    o = O.OracleCCEH(2)
    ost = o.insert(k, np.arange(1, 35, dtype=np.uint64))
    assert np.array_equal(ost, st)
    d, od = t.dump(), o.dump()
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])


def test_reserved_keys_and_capacity():
    t = P.CCEH(depth=1, max_batch=4096, max_segments=3)
    st = t.Insert(np.array([2**64 - 1, 2**64 - 2, 5], np.uint64), np.array([1, 2, 3], np.uint64))
    assert st.tolist() == [P.ST_RESERVED_KEY, P.ST_RESERVED_KEY, P.ST_INSERTED]
    v, s = t.Get(np.array([2**64 - 1, 5, 6], np.uint64))
    assert s.tolist() == [P.ST_RESERVED_KEY, P.ST_HIT, P.ST_MISS] and v[1] == 3
    # 3 segments max: fill until CAPACITY appears, everything else stays exact
    keys = uniform_keys(9, 0, 4000)
    st = t.Insert(keys, keys)
    assert np.any(st == P.ST_CAPACITY)
    ok = st == P.ST_INSERTED
    v, s = t.Get(keys)
    assert np.all(s[ok] == P.ST_HIT) and np.array_equal(v[ok], keys[ok])
    assert t.stats()["segments"] == 3


def test_sharded_instances_reassemble_global_table(scen):
    """Each shard (top 2 hash bits) holds exactly the global serial table's
    segments with that prefix."""
    init_cap, conv, ops, keys, vals = scen["cap256_ins400k"]
    h = P.hash64(keys)
    owner = (h >> np.uint64(62)).astype(np.int64)
    o = O.OracleCCEH(8)
    o.mixed(ops, keys, vals)
    od = o.dump()
    segs_k, segs_v, lds = [], [], []
    for sh in range(4):
        t = P.CCEH(depth=8, shard_bits=2, shard_id=sh, max_batch=1 << 17, max_segments=4096)
        sel = owner == sh
        t.Mixed(ops[sel], keys[sel], vals[sel])
        d = t.dump()
        segs_k.append(d["keys"]); segs_v.append(d["values"]); lds.append(d["local_depth"])
        wrong = t.Mixed(ops[~sel][:10], keys[~sel][:10], vals[~sel][:10])[1]
        assert np.all(wrong == P.ST_WRONG_SHARD)
        t.close()
    assert np.array_equal(np.concatenate(segs_k), od["keys"])
    assert np.array_equal(np.concatenate(segs_v), od["values"])
    assert np.array_equal(np.concatenate(lds), od["local_depth"])


def test_route_by_shard_stable():
    k = P.gen_keys(3, 0, 100000)
    perm, counts = P.route_by_shard(k, 3)
    h = P.hash64(k).cpu().numpy().view(np.uint64)
    own = (h >> np.uint64(61)).astype(np.int64)
    exp = np.argsort(own, kind="stable")
    assert np.array_equal(perm.cpu().numpy(), exp)
    assert counts == np.bincount(own, minlength=8).tolist()


# ---------------------------------------------------------------- bloom
@pytest.fixture(scope="module")
def bloom_golden(golden_dir):
    with open(os.path.join(golden_dir, "bloom.json")) as f:
        return json.load(f)


def test_bloom_bftest(bloom_golden):
    g = bloom_golden["bftest"]
    t = np.arange(10000, dtype=np.uint64) * np.uint64(14)
    b = P.BloomFilter(100000, 2)
    b.add(t[:9999])
    assert S.sha(b.bitmap()) == g["bitmap_sha"]
    qs = np.concatenate([t, uniform_keys(31, 0, 2000)])
    r = b.probe(qs)
    assert np.packbits(r).tobytes().hex() == g["querybb"]
    assert r[0] == 1 and r[9999] == 0  # server/bftest.cpp:32-40


def test_bloom_client_shape_and_fused_get(bloom_golden):
    g = bloom_golden["k4_m1e9"]
    b = P.BloomFilter(1000000000, 4)
    ins = uniform_keys(32, 0, 100000)
    b.add(ins)
    bm = b.bitmap()
    assert S.sha(bm) == g["bitmap_sha"]
    qs = np.concatenate([uniform_keys(32, 0, 20000), uniform_keys(32, 100000, 20000)])
    assert np.packbits(b.probe(qs)).tobytes().hex() == g["querybb"]
    # fused: filtered keys never reach the index; positives get exact Get results
    t = P.CCEH(depth=6, max_batch=1 << 17, max_segments=4096)
    t.Insert(ins, ins ^ np.uint64(1))
    v, s = b.probe_then_get(t, qs)
    pos, _ = O.bloom_check(bm, 1000000000, 4, qs)
    assert np.all((s == P.ST_FILTERED) == (pos == 0))
    gv, gs = t.Get(qs)
    assert np.array_equal(v[pos == 1], gv[pos == 1]) and np.array_equal(s[pos == 1], gs[pos == 1])
    assert np.all(s[:20000] == P.ST_HIT)
    # set_bitmap round trip (bloom_filter_set)
    b2 = P.BloomFilter(1000000000, 4)
    b2.set_bitmap(bm)
    assert np.array_equal(b2.probe(qs), b.probe(qs))


# ------------------------------------------------------- full-size configs
def _insert_stream(t, seed, n, batch):
    for off in range(0, n, batch):
        m = min(batch, n - off)
        k = P.gen_keys(seed, off, m)
        st = t.Insert(k, k)
        assert bool((st == P.ST_INSERTED).all())


def test_config1_16M_matches_oracle():
    """Config 1 shape on the GPU: 16M uniform keys, CCEH_hybrid(16384), value =
    key (server/test_KV.cpp:204-221); whole final table vs the oracle."""
    n = 1 << 24
    t = P.CCEH(16384, max_batch=1 << 20, max_segments=1 << 16)
    _insert_stream(t, 1, n, 1 << 20)
    s = t.stats()
    # the oracle on these keys gives depth 16 / 32,835 segments (the survey's
    # probe, on other random keys, saw 32,833); the dumps are compared below
    assert s["depth"] == 16 and s["segments"] == 32835
    misses = 0
    for off in range(0, n, 1 << 20):
        k = P.gen_keys(1, off, 1 << 20)
        v, st = t.Get(k)
        misses += int(((st != P.ST_HIT) | (v != k)).sum())
    assert misses == 0  # test_KV: 0 failedSearch
    keys = uniform_keys(1, 0, n)
    o = O.OracleCCEH(14, reserve_segments=40000)
    o.insert(keys, keys)
    od, d = o.dump(), t.dump()
    assert d["depth"] == od["depth"]
    assert np.array_equal(d["local_depth"], od["local_depth"])
    assert np.array_equal(d["keys"], od["keys"])
    assert np.array_equal(d["values"], od["values"])
    t.close()


# seed 2: pinned from the oracle on the same keys (build container): depth
# 18, 131,368 segments, 65,832 splits, utilization 49.887 %; seed 1000: the
# bench's own rank-0 stream (bench.py config2), 131,305 segments and 65,769
# splits as its bench lines report -- its whole table is compared with the
# oracle's below like seed 2's
C2_FACTS = {2: (18, 131368, 65832), 1000: (18, 131305, 65769)}


@pytest.mark.parametrize("seed", [2, 1000])
def test_config2_64M_properties(seed):
    """Config 2: 64M uniform keys in 1M insert batches, CCEH_hybrid(65536),
    then 100% Get; structure facts from the reference probe.
    The inserts go through pmdfc_cceh_insert_batches -- the three-buffer
    pipelined entry point bench.py times (the partition of batch i+1 on its
    own stream under batch i's passes) -- with device-resident keys as in the
    bench, and the whole final table is compared with the oracle's."""
    n, B = 1 << 26, 1 << 20
    depth, nseg, nsplit = C2_FACTS[seed]
    t = P.CCEH(65536, max_batch=B, max_segments=1 << 18)
    allk = P.gen_keys(seed, 0, n)
    st = t.InsertBatches(allk, allk, list(range(0, n + 1, B)))
    assert bool((st == P.ST_INSERTED).all())
    del allk, st
    s = t.stats()
    assert s["depth"] == depth and s["segments"] == nseg and s["split_loss"] == 0
    assert s["error_flags"] == 0
    assert s["splits"] == nsplit
    bad = 0
    for off in range(0, n, 1 << 20):
        k = P.gen_keys(seed, off, 1 << 20)
        v, st = t.Get(k)
        bad += int(((st != P.ST_HIT) | (v != k)).sum())
    assert bad == 0
    # the 64 Get batches as one launch (GetBatches, the bench's form), plus
    # absent keys in the last batch: every op's result as batch by batch
    allk = torch.cat([P.gen_keys(seed, 0, n - B), P.gen_keys(seed, n, B)])
    v, st = t.GetBatches(allk, list(range(0, n + 1, B)))
    assert bool((st[:n - B] == P.ST_HIT).all()) and bool((v[:n - B] == allk[:n - B]).all())
    assert bool((st[n - B:] == P.ST_MISS).all()) and bool((v[n - B:] == 0).all())
    del allk, v, st
    absent = P.gen_keys(seed, n, 1 << 20)
    _, st = t.Get(absent)
    assert bool((st == P.ST_MISS).all())
    u = t.Utilization()
    assert abs(u - 100.0 * n / (nseg * 1024)) < 1e-9
    # whole final table, slot for slot, against the oracle on the same keys
    keys = uniform_keys(seed, 0, n)
    o = O.OracleCCEH(16, reserve_segments=140000)
    o.insert(keys, keys)
    del keys
    od = o.dump()
    o.close()
    d = t.dump()
    assert d["depth"] == od["depth"]
    assert np.array_equal(d["local_depth"], od["local_depth"])
    assert np.array_equal(d["keys"], od["keys"])
    assert np.array_equal(d["values"], od["values"])
    t.close()


@pytest.mark.parametrize("depth,batch", [(4, 20000), (2, 65536)])
def test_mixed_early_answers_match_oracle(depth, batch):
    """Gets after their segment's first insert (answered before the batch when
    the batch never inserts their key and the key has one copy): single-copy
    hits, misses, keys with several copies, keys inserted before or after
    the Get in the same batch -- with splits in every batch."""
    rng = np.random.default_rng(depth)
    pre = uniform_keys(300, 0, 30000)
    dup = pre[:300]
    t = P.CCEH(depth=depth, max_batch=batch, max_segments=16384)
    o = O.OracleCCEH(depth)
    base = np.concatenate([pre, dup, dup[:100]])  # 1-3 copies
    t.Insert(base, base ^ np.uint64(7))
    o.insert(base, base ^ np.uint64(7))
    fresh = 0
    for _ in range(4):
        n = batch
        ops = (rng.random(n) < 0.3).astype(np.uint8)
        keys = pre[rng.integers(0, pre.size, n)]
        r = rng.random(n)
        absent = uniform_keys(301, fresh, n)
        keys = np.where(r < 0.15, absent, keys)  # Gets of absent keys; Inserts of fresh ones
        keys = np.where((r > 0.15) & (r < 0.2), dup[rng.integers(0, dup.size, n)], keys)
        inb = np.nonzero(ops == 1)[0]
        later = rng.integers(0, n, inb.size // 4)
        keys[later] = keys[inb[: later.size]]  # Gets of keys this batch inserts (before or after)
        fresh += n
        vals = keys ^ np.uint64(0x55)
        v, s = t.Mixed(ops, keys, vals)
        ov, os_ = o.mixed(ops, keys, vals)
        assert np.array_equal(s, os_) and np.array_equal(v, ov)
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"]
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])
    assert t.stats()["error_flags"] == 0


def test_mixed_read_after_write_in_batch():
    """Gets of keys the same batch inserts once (before or after the Get),
    several times, or that also existed before: exact vs the oracle."""
    rng = np.random.default_rng(9)
    t = P.CCEH(depth=3, max_batch=50000, max_segments=8192)
    o = O.OracleCCEH(3)
    old = uniform_keys(400, 0, 5000)
    t.Insert(old, old)
    o.insert(old, old)
    for b in range(3):
        n = 50000
        fresh = uniform_keys(401 + b, 0, 15000)
        ops = np.zeros(n, np.uint8)
        keys = np.empty(n, np.uint64)
        pos = rng.permutation(n)
        ins = pos[:20000]
        ops[ins] = 1
        keys[ins[:15000]] = fresh                      # once
        keys[ins[15000:17000]] = fresh[:2000]          # twice
        keys[ins[17000:]] = old[rng.integers(0, 5000, 3000)]  # re-insert existing keys
        gets = pos[20000:]
        pick = rng.random(gets.size)
        keys[gets] = np.where(pick < 0.6, fresh[rng.integers(0, 15000, gets.size)],
                              np.where(pick < 0.8, old[rng.integers(0, 5000, gets.size)],
                                       uniform_keys(450 + b, 0, gets.size)))
        vals = keys ^ np.uint64(b + 1)
        v, s = t.Mixed(ops, keys, vals)
        ov, os_ = o.mixed(ops, keys, vals)
        assert np.array_equal(s, os_) and np.array_equal(v, ov), b
    d, od = t.dump(), o.dump()
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])


def test_mixed_zipf_at_scale_vs_oracle():
    """Config-3 shape at a size the oracle finishes in seconds: 2M preloaded
    replay-shape keys, mixed batches of 512k with 95 % Zipf(0.99) Gets and 5 %
    fresh Inserts (hot keys on touched segments, splits in every batch),
    every result and the final table bit-exact vs the serial oracle."""
    from pmdfc_amd.workload import scramble, zipf_ranks
    n_pre, B = 1 << 21, 1 << 19
    rank = np.arange(n_pre + 4 * B, dtype=np.uint64)
    allk = ((np.uint64(1) + (rank >> np.uint64(8))) << np.uint64(32)) + ((rank & np.uint64(255)) << np.uint64(12))
    t = P.CCEH(65536, max_batch=B, max_segments=1 << 14)
    o = O.OracleCCEH(O.OracleCCEH.depth_for_hybrid(65536))
    t.Insert(allk[:n_pre], allk[:n_pre])
    o.insert(allk[:n_pre], allk[:n_pre])
    rng = np.random.default_rng(33)
    fresh = n_pre
    for _ in range(4):
        is_ins = rng.random(B) < 0.05
        r = scramble(zipf_ranks(rng, n_pre, 0.99, B), n_pre, 33)
        nf = int(is_ins.sum())
        r[is_ins] = fresh + np.arange(nf)
        fresh += nf
        keys = allk[r]
        ops = is_ins.astype(np.uint8)
        v, s = t.Mixed(ops, keys, keys)
        ov, os_ = o.mixed(ops, keys, keys)
        assert np.array_equal(s, os_) and np.array_equal(v, ov)
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"]
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])


# ---- Insert4split's silent drop (CCEH_hybrid.cpp:18-28), pinned by the
# reference-generated split_loss fixtures (tests/scenarios.py split_loss)

def _lost_keys(ops, keys, d):
    ins = np.unique(keys[ops == S.OP_INSERT])
    return set(np.setdiff1d(ins, d["keys"]).tolist())


@pytest.mark.parametrize("batch", [0, 997, 65536])
def test_split_loss_insert_get_entry_points(batch, golden, scen, path):
    """Inserts through pmdfc_cceh_insert (k_split / k_bucket's wave_split with
    its loss branch), then Gets: table, Get results and loss count equal the
    reference's, slot for slot."""
    init_cap, conv, ops, keys, vals = scen["split_loss"]
    ins = ops == S.OP_INSERT
    assert ins[: ins.sum()].all()
    t = P.CCEH(init_cap, convention=conv, max_batch=batch or int(ins.sum()), max_segments=8192)
    ik, iv = keys[ins], vals[ins]
    b = batch or ik.size
    st = np.concatenate([t.Insert(ik[o:o + b], iv[o:o + b]) for o in range(0, ik.size, b)])
    assert np.all(st == P.ST_INSERTED)  # the reference reports nothing either (cerr only)
    out, gst = t.Get(keys[~ins])
    full = np.zeros(keys.size, np.uint64)
    full[~ins] = out
    _check(_summary(t, ops, full), golden["split_loss"], "split_loss")
    s = t.stats()
    assert s["split_loss"] == 4 == int(ins.sum()) - golden["split_loss"]["occupied"]
    t.close()


@pytest.mark.parametrize("batch", [0, 997, 65536])
@pytest.mark.parametrize("name", ["split_loss", "split_loss_mixed"])
def test_split_loss_mixed_path(name, batch, golden, scen, path):
    """The same drops inside mixed batches: the final table equals the
    reference's, and EVERY op equals the serial oracle (pinned to the same
    fixture) -- including the Gets answered early, before the batch's inserts,
    whose key a split of the batch dropped: the splits log each drop with the
    insert that triggered them, so k_mixed_verify places the drop before or
    after the Get as the reference does.  No SPLIT_LOST."""
    init_cap, conv, ops, keys, vals = scen[name]
    n = keys.size
    b = batch or n
    t = P.CCEH(init_cap, convention=conv, max_batch=b, max_segments=8192)
    out = np.zeros(n, np.uint64)
    st = np.zeros(n, np.uint8)
    for off in range(0, n, b):
        o, s = t.Mixed(ops[off:off + b], keys[off:off + b], vals[off:off + b])
        out[off:off + b] = o
        st[off:off + b] = s
    d = t.dump()
    g = golden[name]
    for f, v in (("depth", d["depth"]), ("nseg", len(d["local_depth"])),
                 ("keys_sha", S.sha(d["keys"])), ("values_sha", S.sha(d["values"]))):
        assert v == g[f], (name, f)
    o = O.OracleCCEH(t.initial_depth)
    ov, ost = o.mixed(ops, keys, vals)
    assert not np.any(st == P.ST_SPLIT_LOST)
    assert np.array_equal(out, ov) and np.array_equal(st, ost)
    lk = _lost_keys(ops, keys, d)
    assert len(lk) == 4
    s = t.stats()
    assert s["split_loss"] == 4
    assert s["error_flags"] == 0
    t.close()


@pytest.mark.parametrize("batch", [1, 23, 64, 65, 256, 1000, 8192])
@pytest.mark.parametrize("name", ["cap2_ins3k", "cap8_ins20k", "mixed_cap16_60k", "mixed_cap2_30k_ins80", "dup_wrap",
                                  "dup32", "dup_pairs", "src_cap2m_ins50k", "split_loss", "split_loss_mixed"])
def test_small_batches_exact(name, batch, golden, scen):
    """Batches of at most 256 ops take one launch: k_mixed_tiny (<= 64 ops, a
    lane per op, the ordered final-pass runs for shared segments and full
    windows) or k_mixed_small (<= 256, a block per directory bucket); batches
    of at most 8192 take two, k_part's one block and k_medium (the final pass
    over every touched bucket, records in batch order) once the table is at
    full bucket resolution (before that the ramped general pipeline).  All are
    the serial reference exactly: the final table equals the fixture and every
    op's status and value equal the serial oracle's -- including the Gets of
    keys a split drops (no SPLIT_LOST: the ordered runs answer them in place).
    The insert-only entry point takes the same kernels."""
    init_cap, conv, ops, keys, vals = scen[name]
    n = keys.size
    if n > 60000 and batch < 64:
        n = 20000  # (bounded runtime: a prefix of the stream, checked against the oracle alone)
        ops, keys, vals = ops[:n], keys[:n], vals[:n]
    t = P.CCEH(init_cap, convention=conv, max_batch=8192, max_segments=8192)
    out = np.zeros(n, np.uint64)
    st = np.zeros(n, np.uint8)
    all_ins = bool(np.all(ops == S.OP_INSERT))
    for off in range(0, n, batch):
        if all_ins and (off // batch) % 2:
            s = t.Insert(keys[off:off + batch], vals[off:off + batch])
            o = np.zeros(s.size, np.uint64)
        else:
            o, s = t.Mixed(ops[off:off + batch], keys[off:off + batch], vals[off:off + batch])
        out[off:off + batch] = o
        st[off:off + batch] = s
    o = O.OracleCCEH(t.initial_depth)
    ov, ost = o.mixed(ops, keys, vals)
    # (a batch of > 256 ops on a table still coarser than its bucket
    # resolution (CCEH_hybrid(2)) takes the ramped general pipeline: early
    # answers placed through the drop log, exact as well)
    assert np.array_equal(st, ost), name
    assert np.array_equal(out, ov), name
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"] and np.array_equal(d["local_depth"], od["local_depth"])
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])
    if n == scen[name][2].size:
        g = golden[name]
        assert S.sha(d["keys"]) == g["keys_sha"] and S.sha(d["values"]) == g["values_sha"]
    assert t.stats()["error_flags"] == 0
    t.close()


def test_split_loss_get_before_segment_inserts():
    """A Get answered early against the pre-batch image whose key a later split
    of the same batch drops: when the Get precedes every insert of the batch
    into its pre-batch segment, no split of that segment has run yet at its
    turn, so the reference returns the value -- the engine must too (not
    SPLIT_LOST).  Batch 1 stores A and B (scenarios.split_loss); batch 2 reads
    A and B, then inserts C (the split drops 4 of A), then reads A and B again:
    both reads equal the serial oracle exactly (the second misses the 4
    dropped keys: the drop log places their split before it)."""
    a = S._find_keys(13, O.hash64, 248, 0, 36)
    b = S._find_keys(14, O.hash64, 255, 0, 28)
    c, a = a[32:], a[:32]
    ab = np.concatenate([a, b])
    ops = np.concatenate([np.zeros(ab.size, np.uint8), np.ones(c.size, np.uint8), np.zeros(ab.size, np.uint8)])
    keys = np.concatenate([ab, c, ab])
    vals = np.where(ops == S.OP_INSERT, keys ^ np.uint64(0x1234), np.uint64(0)).astype(np.uint64)
    t = P.CCEH(2, max_batch=1024, max_segments=64)
    assert np.all(t.Insert(ab, ab ^ np.uint64(0x1234)) == P.ST_INSERTED)
    out, st = t.Mixed(ops, keys, vals)
    o = O.OracleCCEH(t.initial_depth)
    o.insert(ab, ab ^ np.uint64(0x1234))
    ov, ost = o.mixed(ops, keys, vals)
    assert o.stats()["split_loss"] == 4 and t.stats()["split_loss"] == 4
    first = np.arange(ab.size)
    assert np.all(ost[first] == P.ST_HIT)
    assert int((ost[ab.size + c.size:] == P.ST_MISS).sum()) == 4
    assert np.array_equal(out, ov) and np.array_equal(st, ost)
    assert t.stats()["error_flags"] == 0
    t.close()


@pytest.mark.parametrize("order", ["drop_then_reinsert", "reinsert_then_drop"])
def test_unchecked_early_hits_dropped_and_reinserted(order):
    """Early hits answered without the inserted-key set (a non-wrapping
    window: A's home line 248) whose key a split of the same batch drops and
    the batch inserts again.  Batch 1 stores A and B; batch 2 (the general
    pipeline: > 256 ops on a ramping table) reads A and B, then either inserts
    C (the split drops 4 of A) and A again with new values, or A again first
    (two copies of each A key, so the split drops more) and then C, then reads
    A and B; absent-key Gets pad the batch.  Every op equals the serial
    oracle: k_mixed_verify replays such a key's copies from the drop log and
    the batch's stored inserts (cceh_kernels.hip replay_unchecked_hit)."""
    a = S._find_keys(13, O.hash64, 248, 0, 36)
    b = S._find_keys(14, O.hash64, 255, 0, 28)
    c, a = a[32:], a[:32]
    ab = np.concatenate([a, b])
    pad = S.uniform_keys(99, 0, 300)
    parts = [(S.OP_GET, ab)]
    if order == "drop_then_reinsert":
        parts += [(S.OP_INSERT, c), (S.OP_GET, a), (S.OP_INSERT, a), (S.OP_GET, ab)]
    else:
        parts += [(S.OP_INSERT, a), (S.OP_GET, a), (S.OP_INSERT, c), (S.OP_GET, ab)]
    parts += [(S.OP_GET, pad), (S.OP_GET, ab)]
    ops = np.concatenate([np.full(k.size, o, np.uint8) for o, k in parts])
    keys = np.concatenate([k for _, k in parts])
    vals = np.where(ops == S.OP_INSERT, keys ^ np.uint64(0x5678) ^ np.arange(keys.size, dtype=np.uint64),
                    np.uint64(0)).astype(np.uint64)
    assert ops.size > 256
    t = P.CCEH(2, max_batch=1024, max_segments=64)
    assert np.all(t.Insert(ab, ab ^ np.uint64(0x1234)) == P.ST_INSERTED)
    out, st = t.Mixed(ops, keys, vals)
    o = O.OracleCCEH(t.initial_depth)
    o.insert(ab, ab ^ np.uint64(0x1234))
    ov, ost = o.mixed(ops, keys, vals)
    assert o.stats()["split_loss"] > 0 and t.stats()["split_loss"] == o.stats()["split_loss"]
    assert np.array_equal(st, ost) and np.array_equal(out, ov)
    d, od = t.dump(), o.dump()
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])
    assert t.stats()["error_flags"] == 0
    t.close()


# ---- last-writer-wins (upsert) mode, pinned by the reference's
# CCEH_hybrid.cpp with its overwrite clause (:153) enabled
# (oracle/CCEH_hybrid.upsert.patch, tests/golden/upsert_scenarios.json)

UPSERT_NAMES = ["up_dup_wrap", "up_dup_many", "up_dup_pairs", "up_reinserts_cap2", "up_reinserts_cap256",
                "up_split_loss_mixed"]


@pytest.fixture(scope="module")
def upsert_golden(golden_dir):
    with open(os.path.join(golden_dir, "upsert_scenarios.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def upsert_scen():
    return S.upsert_scenarios(O.hash64)


@pytest.mark.parametrize("batch", [0, 997, 65536])
@pytest.mark.parametrize("name", UPSERT_NAMES)
def test_upsert_mixed_matches_reference(name, batch, upsert_golden, upsert_scen, path):
    init_cap, conv, ops, keys, vals = upsert_scen[name]
    n = keys.size
    b = batch or n
    t = P.CCEH(init_cap, convention=conv, max_batch=b, max_segments=8192, upsert=True)
    out = np.zeros(n, np.uint64)
    st = np.zeros(n, np.uint8)
    for off in range(0, n, b):
        o, s = t.Mixed(ops[off:off + b], keys[off:off + b], vals[off:off + b])
        out[off:off + b] = o
        st[off:off + b] = s
    g = upsert_golden[name]
    o = O.OracleCCEH(t.initial_depth, upsert=True)
    ov, ost = o.mixed(ops, keys, vals)
    assert np.array_equal(out, ov) and np.array_equal(st, ost)  # (no SPLIT_LOST: the drop log places drops)
    _check(_summary(t, ops, out), g, name)
    ins = ops == S.OP_INSERT
    assert int((st[ins] == P.ST_UPDATED).sum()) == int((ost[ins] == O.ST_UPDATED).sum())
    assert abs(t.Utilization() - g["utilization"]) < 1e-9
    t.close()


@pytest.mark.parametrize("batch", [23, 200, 3000])
def test_upsert_small_batches_exact(batch, upsert_golden, upsert_scen):
    """Last-writer-wins through the one- and two-launch paths (k_mixed_tiny:
    every upsert insert takes the ordered runs; k_mixed_small; k_medium): every
    op equal to the serial reference with its overwrite clause (oracle), the
    final table equal to the fixture."""
    for name in sorted(upsert_scen):
        init_cap, conv, ops, keys, vals = upsert_scen[name]
        n = keys.size
        t = P.CCEH(init_cap, convention=conv, max_batch=8192, max_segments=8192, upsert=True)
        out = np.zeros(n, np.uint64)
        st = np.zeros(n, np.uint8)
        for off in range(0, n, batch):
            o, s = t.Mixed(ops[off:off + batch], keys[off:off + batch], vals[off:off + batch])
            out[off:off + batch] = o
            st[off:off + batch] = s
        o = O.OracleCCEH(t.initial_depth, upsert=True)
        ov, ost = o.mixed(ops, keys, vals)
        assert np.array_equal(out, ov) and np.array_equal(st, ost), name
        _check(_summary(t, ops, out), upsert_golden[name], name)
        t.close()


@pytest.mark.parametrize("batch", [997, 65536])
def test_upsert_insert_entry_point(batch, upsert_golden, upsert_scen, path):
    """Insert-only upsert batches (pmdfc_cceh_insert: k_apply's general run
    loop with the key probe, in-run claims of the same key merged), then Gets."""
    init_cap, conv, ops, keys, vals = upsert_scen["up_dup_pairs"]
    ins = ops == S.OP_INSERT
    assert ins[: ins.sum()].all()
    t = P.CCEH(init_cap, convention=conv, max_batch=batch, max_segments=8192, upsert=True)
    ik, iv = keys[ins], vals[ins]
    st = np.concatenate([t.Insert(ik[o:o + batch], iv[o:o + batch]) for o in range(0, ik.size, batch)])
    o = O.OracleCCEH(t.initial_depth, upsert=True)
    ost = o.insert(ik, iv)
    assert np.array_equal(st, ost)
    out, gst = t.Get(keys[~ins])
    full = np.zeros(keys.size, np.uint64)
    full[~ins] = out
    _check(_summary(t, ops, full), upsert_golden["up_dup_pairs"], "up_dup_pairs")
    t.close()


def test_upsert_same_key_inside_one_run():
    """Many inserts of a few keys inside one batch (each run of a segment holds
    several claims of one key): the last value wins and the key keeps one slot."""
    rng = np.random.default_rng(5)
    base = uniform_keys(61, 0, 64)
    keys = base[rng.integers(0, 64, 20000)]
    vals = np.arange(1, 20001, dtype=np.uint64)
    t = P.CCEH(depth=2, max_batch=1 << 15, max_segments=256, upsert=True)
    st = t.Insert(keys, vals)
    o = O.OracleCCEH(2, upsert=True)
    assert np.array_equal(st, o.insert(keys, vals))
    v, s = t.Get(base)
    ov, os_ = o.get(base)
    assert np.array_equal(v, ov) and np.array_equal(s, os_)
    d = t.dump()
    occ = d["keys"][d["keys"] != np.uint64(2**64 - 1)]
    assert occ.size == 64 and np.unique(occ).size == 64
    t.close()


def test_small_table_rebuckets_and_matches_oracle():
    """CCEH_hybrid(2) (NUMA_KV's default geometry): the engine starts with 2
    directory buckets and re-buckets as the segments deepen (k_rebucket at a
    batch start, decided from the live-segment depth counts without a host
    wait); inserts then Gets in batches stay bit-exact with the serial oracle."""
    B, n = 8192, 300000
    keys = np.array(S.uniform_keys(77, 0, n), dtype=np.uint64)
    vals = S._vals(keys)
    t = P.CCEH(2, max_batch=1 << 16, max_segments=4096)
    o = O.OracleCCEH(O.OracleCCEH.depth_for_hybrid(2))
    assert t.stats()["bucket_bits"] == 1
    for i in range(0, n, B):
        st = t.Insert(keys[i:i + B], vals[i:i + B])
        assert np.array_equal(st, o.insert(keys[i:i + B], vals[i:i + B]))
    s = t.stats()
    assert s["bucket_bits"] > 4, s  # re-bucketed several times
    for i in range(0, n, 1 << 16):
        v, st = t.Get(keys[i:i + (1 << 16)])
        ov, os_ = o.get(keys[i:i + (1 << 16)])
        assert np.array_equal(st, os_) and np.array_equal(v, ov)
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"]
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])
    t.close()


@pytest.mark.parametrize("mixed", [False, True])
def test_general_and_medium_batches_alternate(mixed):
    """Batches above and at or below 8,192 ops alternate on a table at its
    bucket resolution, with splits in every batch: the medium path (k_part's
    one block + k_medium, splits inline) must leave the general path's
    per-batch words (grant shards, worklists, by batch parity) as the next
    general batch expects them.  Every status and value and the final table
    equal the serial oracle."""
    rng = np.random.default_rng(44 + mixed)
    t = P.CCEH(depth=7, max_batch=1 << 14, max_segments=1 << 12)  # p1max = 7: at resolution from the start
    o = O.OracleCCEH(7)
    # a preload to ~45 % load, then splits in every batch
    sizes = [16384] * 4 + [5000, 12000, 8192, 16384, 300, 14000, 8191, 16000, 64, 16000, 6000, 16384, 7000, 15000]
    fresh = 0
    stored = np.zeros(0, np.uint64)
    for b in sizes:
        k = uniform_keys(500, fresh, b)
        fresh += b
        if mixed and stored.size:
            ops = (rng.random(b) < 0.6).astype(np.uint8)
            g = ops == 0
            k[g] = np.where(rng.random(int(g.sum())) < 0.8, stored[rng.integers(0, stored.size, int(g.sum()))], k[g])
            v = k ^ np.uint64(0x77)
            out, st = t.Mixed(ops, k, v)
            oout, ost = o.mixed(ops, k, v)
            assert np.array_equal(out, oout), b
            stored = np.concatenate([stored, k[ops == 1]])
        else:
            v = k ^ np.uint64(0x77)
            st = t.Insert(k, v)
            ost = o.insert(k, v)
            stored = np.concatenate([stored, k])
        assert np.array_equal(st, ost), b
    s = t.stats()
    assert s["error_flags"] == 0 and s["splits"] > 100
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"] and np.array_equal(d["local_depth"], od["local_depth"])
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])
    t.close()


@pytest.mark.parametrize("mixed", [False, True])
def test_wide_first_pass_matches_oracle(mixed):
    """A table with more than 20 segments per directory bucket (2^7 buckets
    at max_batch 16,384; ~45 at the end) takes the lean first pass in its wide
    variant (k_apply_wide: sub-directories up to 128 entries in their fixed
    slots, bins assigned to the touched segments): every status, every Get and
    the final table equal the serial oracle, and the fast passes decline few
    buckets (a table the narrow pass cannot take would decline all)."""
    rng = np.random.default_rng(71 + mixed)
    B, Bm = 1 << 14, 12000  # (mixed/insert batches of 12,000: ~94 inserts per bucket, within the wide pass's 128)
    t = P.CCEH(depth=7, max_batch=B, max_segments=1 << 14)
    o = O.OracleCCEH(7)
    n_pre = 3 << 20
    keys = uniform_keys(600, 0, n_pre)
    for off in range(0, n_pre, B):
        k = keys[off:off + B]
        assert np.array_equal(t.Insert(k, k ^ np.uint64(5)), o.insert(k, k ^ np.uint64(5)))
    s0 = t.stats()
    assert s0["segments"] >> s0["bucket_bits"] > 20, s0
    fresh = n_pre
    for _ in range(12):
        if mixed:
            ops = (rng.random(Bm) < 0.5).astype(np.uint8)
            k = np.where(ops == 1, uniform_keys(600, fresh, Bm), keys[rng.integers(0, n_pre, Bm)])
            fresh += Bm
            v = k ^ np.uint64(5)
            out, st = t.Mixed(ops, k, v)
            oout, ost = o.mixed(ops, k, v)
            assert np.array_equal(out, oout) and np.array_equal(st, ost)
        else:
            k = uniform_keys(600, fresh, Bm)
            fresh += Bm
            assert np.array_equal(t.Insert(k, k ^ np.uint64(5)), o.insert(k, k ^ np.uint64(5)))
    s = t.stats()
    assert s["error_flags"] == 0
    # the fast passes took most buckets of the last batches (the hint lags a little)
    assert s["fast_declined"] - s0["fast_declined"] < 12 * (1 << s["bucket_bits"]) // 4, (s0, s)
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"] and np.array_equal(d["local_depth"], od["local_depth"])
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])
    t.close()


def _interleave_steps():
    """The call sequence of test_batch_kinds_interleave_on_one_table: (kind,
    sizes) with fresh keys uniform_keys(700, ...) consumed in order."""
    return [("batches", [65536] * 9),  # preload: one full pipeline group and a group of one
            ("insert", 40000), ("mixed", 30000), ("insert", 40000),
            ("batches", [40000, 0, 20000, 65536]),
            ("insert", 5000),  # medium
            ("insert", 40000),
            ("mixed", 200),  # small
            ("mixed", 6000),  # medium
            ("mixed", 40000),
            ("batches", [30000, 30000])]


def test_batch_kinds_interleave_on_one_table():
    """Every batch kind on ONE table with no reset in between: pipelined
    groups (pmdfc_cceh_insert_batches), general insert and mixed batches,
    medium and small ones.  The table (p1max = 9) is at its bucket resolution
    from the start, so insert-only batches past 8,192 ops take the coarse
    partition and mixed ones the fine one: the record-buffer ring, the batch
    parity and the cursors a batch leaves zeroed for the next one's geometry
    carry over between the paths.  Every status and value, the final table
    and the Gets of every stored key equal the serial oracle."""
    rng = np.random.default_rng(9)
    t = P.CCEH(depth=10, max_batch=1 << 16, max_segments=8192)
    o = O.OracleCCEH(10)
    fresh = 0
    stored = np.zeros(0, np.uint64)
    for step, (kind, sizes) in enumerate(_interleave_steps()):
        n = sum(sizes) if kind == "batches" else sizes
        k = uniform_keys(700, fresh, n)
        fresh += n
        if kind == "mixed":
            ops = (rng.random(n) < 0.6).astype(np.uint8)
            g = ops == 0
            k[g] = np.where(rng.random(int(g.sum())) < 0.8, stored[rng.integers(0, stored.size, int(g.sum()))], k[g])
            v = k ^ np.uint64(3)
            out, st = t.Mixed(ops, k, v)
            oout, ost = o.mixed(ops, k, v)
            assert np.array_equal(out, oout), step
            stored = np.concatenate([stored, k[ops == 1]])
        else:
            v = k ^ np.uint64(3)
            if kind == "batches":
                st = t.InsertBatches(k, v, np.concatenate([[0], np.cumsum(sizes)]).tolist())
            else:
                st = t.Insert(k, v)
            ost = o.insert(k, v)
            stored = np.concatenate([stored, k])
        assert np.array_equal(st, ost), step
    v, st = t.Get(stored)
    ov, ost = o.get(stored)
    assert np.array_equal(st, ost) and np.array_equal(v, ov)
    s = t.stats()
    assert s["error_flags"] == 0
    assert s["splits"] > 900
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"] and np.array_equal(d["local_depth"], od["local_depth"])
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])
    t.close()


def test_debug_stamps_follow_the_batch(monkeypatch):
    """PMDFC_STAMPS=1 (a create knob): the stamps pmdfc_cceh_debug_stamps
    returns are those of the LAST batch, through the one-batch path and through
    the pipelined one.  A 40,000-op batch has five k_part blocks, each stamping
    its start (word 0) and end (word 3); every first-pass wave stamps phase 0
    of its bucket's row; the counter is a wall clock, so a later batch's
    stamps are greater."""
    monkeypatch.setenv("PMDFC_STAMPS", "1")
    t = P.CCEH(depth=10, max_batch=1 << 16, max_segments=8192)
    keys = uniform_keys(701, 0, 100000)
    vals = keys ^ np.uint64(3)
    assert np.all(t.Insert(keys[:40000], vals[:40000]) == P.ST_INSERTED)
    bk, pt, sp = t.debug_stamps(1 << 16)
    assert bk.shape == (512, 16) and pt.shape == (8, 8)
    assert np.all(pt[:5, 0] > 0) and np.all(pt[:5, 3] >= pt[:5, 0])
    assert np.all(pt[5:] == 0)  # (zeroed at create, never written by a five-block batch)
    assert np.all(bk[:, 0] > 0)
    bk, pt = bk.copy(), pt.copy()
    # the pipelined path: its last batch (40,000 ops again) owns the set read
    assert np.all(t.InsertBatches(keys[40000:], vals[40000:], [0, 20000, 60000]) == P.ST_INSERTED)
    bk2, pt2, sp2 = t.debug_stamps(1 << 16)
    assert np.all(pt2[:5, 0] > pt[:5, 3])
    assert np.all(bk2[:, 0] > bk[:, 0])
    assert t.stats()["error_flags"] == 0
    t.close()


# One insert-only stream per first-pass variant, each in a child process (the
# engine reads PMDFC_CP / PMDFC_FAST_APPLY once per process): 40 batches of
# 20,000 fresh keys into CCEH_hybrid(8), so the table ramps through every
# bucket resolution (splits and sub-directory growth in every batch) up to
# its full 2^9 buckets (max_batch 65,536), where a 20,000-op batch is
# eligible for the coarse partition and the default takes k_apply_fast_cp.
_FIRST_PASS_CHILD = r'''
import json, sys, numpy as np
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys
import pmdfc_amd as P
B, nb = 20000, 40
t = P.CCEH(8, max_batch=1 << 16, max_segments=4096)
o = O.OracleCCEH(t.initial_depth)
ok = True
for i in range(nb):
    k = uniform_keys(810, i * B, B)
    ok = ok and bool(np.array_equal(t.Insert(k, k ^ np.uint64(9)), o.insert(k, k ^ np.uint64(9))))
d, od = t.dump(), o.dump()
ok = ok and d["depth"] == od["depth"] and all(np.array_equal(d[f], od[f]) for f in ("local_depth", "keys", "values"))
s, os_ = t.stats(), o.stats()
print(json.dumps({"ok": ok, "stats": {k: int(v) for k, v in s.items()},
                  "oracle": {"segments": o.num_segments, "depth": o.depth, "splits": int(os_["splits"]),
                             "split_loss": int(os_["split_loss"])}}))
t.close()
'''
_FIRST_PASS_ENVS = {"default": {}, "cp0": {"PMDFC_CP": "0"}, "fast_apply0": {"PMDFC_FAST_APPLY": "0"}}


def test_first_pass_variants_keep_the_same_books():
    """The lean first pass with the coarse partition (default), with the fine
    one (PMDFC_CP=0) and the general first pass (PMDFC_FAST_APPLY=0) share
    their prologue and their stat epilogue: each leaves the oracle's table and
    the same path-independent stats (those the oracle keeps equal the
    oracle's; "doublings" counts sub-directory growths, which the reference's
    single directory does not have, so it is compared between the variants
    only).  The path-dependent counters are printed, not compared."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = {}
    for name, env in _FIRST_PASS_ENVS.items():
        e = dict(os.environ)
        for k in ("PMDFC_CP", "PMDFC_FAST_APPLY", "PMDFC_CHUNK", "PMDFC_P1MAX"):
            e.pop(k, None)
        e.update(env)
        procs[name] = subprocess.Popen([sys.executable, "-c", _FIRST_PASS_CHILD], cwd=repo, env=e,
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    res = {}
    for name, p in procs.items():
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, (name, err[-2000:])
        res[name] = json.loads(out.strip().splitlines()[-1])
    for name, r in res.items():
        print(name, {k: r["stats"][k] for k in ("insert_lines", "segment_runs", "insert_passes", "deferred_ops",
                                                "max_rounds", "fast_declined")})
    same = ("segments", "depth", "splits", "doublings", "split_loss", "batches", "error_flags", "bucket_bits")
    ref = res["default"]
    assert ref["stats"]["bucket_bits"] == 9, ref["stats"]  # at full resolution: the last batches took the coarse partition
    for name, r in res.items():
        assert r["ok"], name  # every status and the final table equal the oracle's
        assert r["stats"]["error_flags"] == 0, name
        assert r["stats"]["splits"] > 200, (name, r["stats"])  # the stream did split and grow
        assert r["stats"]["doublings"] > 0, (name, r["stats"])
        for k in same:
            assert r["stats"][k] == ref["stats"][k], (name, k, r["stats"][k], ref["stats"][k])
        for k, v in r["oracle"].items():
            assert r["stats"][k] == v, (name, k, r["stats"][k], v)


def test_every_chunk_loader_on_one_table(monkeypatch):
    """Every way a bucket pass loads its chunk, on one small table with
    64-op chunks (PMDFC_CHUNK, read at create): a 20,000-op insert batch whose
    buckets overflow their chunk (the final pass's tile walk: whole tiles and
    the in-tile map), mixed and insert batches that park ops behind splits
    (the parked lists of the parked and the final pass), an 8,192-op batch
    (k_medium: pre-marked big buckets) and a 200-op mixed batch (k_mixed_small:
    the chunk loaded by the caller).  Every status and value after each batch
    and the final table equal the serial oracle."""
    monkeypatch.setenv("PMDFC_CHUNK", "64")
    monkeypatch.delenv("PMDFC_P1MAX", raising=False)
    rng = np.random.default_rng(31)
    t = P.CCEH(depth=5, max_batch=20000, max_segments=4096)
    o = O.OracleCCEH(5)
    steps = [("insert", 20000), ("mixed", 12000), ("insert", 12000), ("insert", 20000), ("mixed", 20000),
             ("insert", 9000), ("insert", 8192), ("mixed", 8192), ("mixed", 200), ("insert", 256)]
    fresh = 0
    stored = np.zeros(0, np.uint64)
    for step, (kind, n) in enumerate(steps):
        k = uniform_keys(811, fresh, n)
        fresh += n
        s0 = t.stats()["splits"]
        if kind == "mixed":
            ops = (rng.random(n) < 0.6).astype(np.uint8)
            g = ops == 0
            k[g] = np.where(rng.random(int(g.sum())) < 0.8, stored[rng.integers(0, stored.size, int(g.sum()))], k[g])
            v = k ^ np.uint64(3)
            out, st = t.Mixed(ops, k, v)
            oout, ost = o.mixed(ops, k, v)
            assert np.array_equal(out, oout), step
            stored = np.concatenate([stored, k[ops == 1]])
        else:
            v = k ^ np.uint64(3)
            st = t.Insert(k, v)
            ost = o.insert(k, v)
            stored = np.concatenate([stored, k])
        assert np.array_equal(st, ost), step
        print(step, kind, n, "splits", t.stats()["splits"] - s0)
    v, st = t.Get(stored)
    ov, ost = o.get(stored)
    assert np.array_equal(st, ost) and np.array_equal(v, ov)
    s = t.stats()
    assert s["error_flags"] == 0
    # (the stored keys need at least size / 1024 segments, each past the first 32 made by a split)
    assert s["splits"] == o.stats()["splits"] and s["splits"] >= -(-stored.size // 1024) - 32
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"] and np.array_equal(d["local_depth"], od["local_depth"])
    assert np.array_equal(d["keys"], od["keys"]) and np.array_equal(d["values"], od["values"])
    t.close()
