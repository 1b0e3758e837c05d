"""pmdfc_cbf_rebuild / pmdfc_cbf_audit on the GPU: the counting
bloom filter from the table's stored keys.

Nothing expected here comes from the code under test: the table is the serial
oracle's (OracleCCEH over the same stream), the stored keys are its dump's
keys != INVALID, and the counters are OracleCBF(m, k).insert of those keys.
"""
import os
import subprocess

import numpy as np
import pytest

import scenarios as S
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pmdfc_amd as P  # noqa: E402
from pmdfc_amd import image as I  # noqa: E402
from pmdfc_amd.kv import KV  # noqa: E402

INVALID = np.uint64(2**64 - 1)
STREAMS = ["cap2_ins3k", "dup32", "dup_wrap", "split_loss"]
# m no multiple of 4, of 64 or of 4,096 (the pack step), k no multiple of 4;
# m = 64: every lane of a wave meets the others in 16 words
FILTERS = [(64, 4), (4099, 3), (100003, 5)]


@pytest.fixture(scope="module")
def scen():
    return S.scenarios(O.hash64)


def _depth(init_cap, conv):
    return O.OracleCCEH.depth_for_hybrid(init_cap) if conv == "hybrid" else O.OracleCCEH.depth_for_src(init_cap)


def live_keys(dump) -> np.ndarray:
    return dump["keys"][dump["keys"] != INVALID]


def want_counters(m, k, *key_sets) -> np.ndarray:
    o = O.OracleCBF(m, k)
    for ks in key_sets:
        o.insert(ks)
    return o.counters.copy()


@pytest.fixture(scope="module")
def serial(scen):
    """name -> (initial depth, the oracle's stored keys after the whole stream,
    its dropped entries), computed once and left unchanged."""
    out = {}
    for name in STREAMS:
        init_cap, conv, ops, keys, vals = scen[name]
        d0 = _depth(init_cap, conv)
        o = O.OracleCCEH(d0)
        o.mixed(ops, keys, vals)
        out[name] = (d0, live_keys(o.dump()), o.stats()["split_loss"])
    return out


def filled(init_cap, conv, ops, keys, vals, **kw):
    t = P.CCEH(init_cap, convention=conv, max_batch=4096, max_segments=256, **kw)
    for lo in range(0, len(ops), 4096):
        t.Mixed(ops[lo:lo + 4096], keys[lo:lo + 4096], vals[lo:lo + 4096])
    return t


def header_live(t) -> int:
    return I.validate(t.snapshot().cpu().numpy().tobytes())["live"]


# ---- 1. the fixture streams, bit-exact

@pytest.mark.parametrize("name", STREAMS)
def test_rebuild_equals_oracle(name, scen, serial):
    init_cap, conv, ops, keys, vals = scen[name]
    d0, live, loss = serial[name]
    t = filled(init_cap, conv, ops, keys, vals)
    assert np.array_equal(np.sort(live_keys(t.dump())), np.sort(live))
    if name == "split_loss":
        assert loss == 4 == int((ops == P.OP_INSERT).sum()) - live.size  # the dropped entries are not stored
    if name == "dup32":
        u, c = np.unique(live, return_counts=True)
        assert c.max() == 32  # 32 stored copies of one key: +32 on its indices
    for m, k in FILTERS:
        f = P.CountingBloomFilter(k, m)
        f.Insert(uniform_keys(5, 0, 100))  # (cleared by the rebuild)
        f.ToOrdinaryBloomFilter()
        stored = f.rebuild(t)
        assert stored == live.size == header_live(t), (name, m, k)
        assert not f.bitmap().any()  # the packed bitmap is cleared with the counters
        assert np.array_equal(f.counters(), want_counters(m, k, live)), (name, m, k)
        assert f.audit(t) == (stored, 0)
        f.close()
    t.close()


# ---- 2. exact saturation

def test_rebuild_saturates_exactly():
    m, k = 64, 4
    keys = uniform_keys(7, 0, 4000)
    o = O.OracleCCEH(1)
    o.insert(keys, keys)
    live = live_keys(o.dump())
    want = want_counters(m, k, live)
    assert o.num_segments == 8 and int((want == 255).sum()) == 22 and want.min() >= 216
    t = P.CCEH(depth=1, max_batch=4096, max_segments=64)
    t.Insert(keys, keys)
    f = P.CountingBloomFilter(k, m)
    assert f.rebuild(t) == live.size
    assert np.array_equal(f.counters(), want)
    t.close()
    keys = uniform_keys(7, 0, 20000)
    o = O.OracleCCEH(4)
    o.insert(keys, keys)
    live = live_keys(o.dump())
    assert np.all(want_counters(m, k, live) == 255)
    t = P.CCEH(depth=4, max_batch=1 << 15, max_segments=256)
    t.Insert(keys, keys)
    assert f.rebuild(t) == live.size
    assert np.all(f.counters() == 255)  # no carry into a neighbour, no wrap
    assert f.rebuild(t, keep=True) == live.size
    assert np.all(f.counters() == 255)
    f.close()
    t.close()


# ---- 3. edges

def test_rebuild_empty_one_key_and_reset():
    m, k = 4099, 3
    t = P.CCEH(depth=1, max_batch=4096, max_segments=64)
    f = P.CountingBloomFilter(k, m)
    f.Insert(uniform_keys(11, 0, 500))
    f.ToOrdinaryBloomFilter()
    assert f.counters().any() and f.bitmap().any()
    assert f.rebuild(t) == 0  # an empty table of 2 segments
    assert not f.counters().any() and not f.bitmap().any()
    assert f.audit(t) == (0, 0)
    one = np.array([0x1234567], np.uint64)
    t.Insert(one, one)
    assert f.rebuild(t) == 1
    assert np.array_equal(f.counters(), want_counters(m, k, one))
    more = uniform_keys(12, 0, 3000)
    t.Insert(more, more)
    assert f.rebuild(t) == 3001
    t.reset()
    assert f.rebuild(t) == 0 and not f.counters().any()  # segments past nsegs still hold the old keys
    t.Insert(one, one)
    assert f.rebuild(t) == 1
    assert np.array_equal(f.counters(), want_counters(m, k, one))
    f.close()
    t.close()


def test_rebuild_never_reads_the_stale_arena():
    """Eight segments of keys, then the image of a one-key table over them:
    arena ids 2..7 keep their old pairs and lie past nsegs."""
    m, k = 100003, 5
    old = uniform_keys(13, 0, 3000)
    o = O.OracleCCEH(1)
    o.insert(old, old)
    assert o.num_segments == 8
    one = np.array([0xABCDEF01], np.uint64)
    o1 = O.OracleCCEH(1)
    o1.insert(one, one)
    img = I.image_from_dump(o1.dump(), 1)
    t = P.CCEH(depth=1, max_batch=4096, max_segments=64)
    t.Insert(old, old)
    assert t.stats()["segments"] == 8
    t.restore(img)
    f = P.CountingBloomFilter(k, m)
    assert f.rebuild(t) == 1
    want = want_counters(m, k, one)
    assert want.max() == 1 and int(want.sum()) == k
    assert np.array_equal(f.counters(), want)
    f.close()
    t.close()


# ---- 4. ordering on the stream

def test_rebuild_follows_a_splitting_batch_without_a_host_sync():
    m, k = 4099, 3
    keys = uniform_keys(14, 0, 4000)
    o = O.OracleCCEH(1)
    o.insert(keys, keys)
    live = live_keys(o.dump())
    assert o.stats()["splits"] > 0
    t = P.CCEH(depth=1, max_batch=4096, max_segments=64)
    f = P.CountingBloomFilter(k, m)
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    torch.cuda.synchronize()
    t.Insert(dk, dk)  # device tensors in, device statuses out: nothing waits
    stored = f.rebuild(t)
    assert stored == live.size
    assert np.array_equal(f.counters(), want_counters(m, k, live))
    f.close()
    t.close()


# ---- 5. KEEP: shards into one filter

def test_keep_adds_shards_into_one_filter():
    m, k = 4099, 3
    keys = uniform_keys(15, 0, 20000)
    o = O.OracleCCEH(3)
    o.insert(keys, keys)
    live = live_keys(o.dump())
    want = want_counters(m, k, live)
    owner = (O.hash64(keys) >> np.uint64(62)).astype(np.int64)
    perm, counts = P.route_by_shard(torch.from_numpy(keys.view(np.int64)).cuda(), 2)
    assert np.array_equal(np.asarray(counts), np.bincount(owner, minlength=4))
    perm = perm.cpu().numpy().astype(np.int64)
    f = P.CountingBloomFilter(k, m)
    f.Insert(uniform_keys(5, 0, 100))
    total, lo = 0, 0
    shards = []
    for sh in range(4):
        sel = perm[lo:lo + int(counts[sh])]
        lo += int(counts[sh])
        assert np.all(owner[sel] == sh)
        t = P.CCEH(depth=3, shard_bits=2, shard_id=sh, max_batch=1 << 15, max_segments=256)
        assert np.all(t.Insert(keys[sel], keys[sel]) == P.ST_INSERTED)
        total += f.rebuild(t, keep=sh > 0)  # the first clears, the others add
        shards.append(t)
    assert total == live.size
    assert np.array_equal(f.counters(), want)
    one = P.CCEH(depth=3, max_batch=1 << 15, max_segments=256)
    one.Insert(keys, keys)
    g = P.CountingBloomFilter(k, m)
    assert g.rebuild(one) == live.size
    assert np.array_equal(g.counters(), want)
    # KEEP twice on one table: the doubled multiset
    mine = live_keys(shards[0].dump())
    assert g.rebuild(shards[0]) == mine.size
    assert g.rebuild(shards[0], keep=True) == mine.size
    assert np.array_equal(g.counters(), want_counters(m, k, mine, mine))
    for t in shards + [one]:
        t.close()
    f.close()
    g.close()


# ---- 6. maintained against rebuilt

def test_maintained_and_rebuilt_filters_are_identical(scen, serial):
    init_cap, conv, ops, keys, vals = scen["cap2_ins3k"]
    d0, live, loss = serial["cap2_ins3k"]
    ins = keys[ops == P.OP_INSERT]
    assert loss == 0 and np.unique(ins).size == ins.size == live.size  # duplicate-free, no drops
    t = filled(init_cap, conv, ops, keys, vals)
    for m, k in FILTERS:
        a, b = P.CountingBloomFilter(k, m), P.CountingBloomFilter(k, m)
        a.Insert(ins)
        b.rebuild(t)
        assert np.array_equal(a.counters(), b.counters())
        a.ToOrdinaryBloomFilter()
        b.ToOrdinaryBloomFilter()
        assert np.array_equal(a.bitmap(), b.bitmap())
        o = O.OracleCBF(m, k)
        o.insert(live)
        assert np.array_equal(b.counters(), o.counters) and np.array_equal(b.bitmap(), o.bitmap())
        a.close()
        b.close()
    t.close()


# ---- 7. audit

def test_audit_counts_the_keys_a_client_would_never_ask_for(scen, serial):
    init_cap, conv, ops, keys, vals = scen["dup_wrap"]
    d0, live, loss = serial["dup_wrap"]
    t = filled(init_cap, conv, ops, keys, vals)
    m, k = 100003, 5
    f = P.CountingBloomFilter(k, m)
    assert f.audit(t) == (live.size, live.size)  # a fresh filter denies every stored entry
    half = np.unique(live)[::2]
    f.Insert(half)
    o = O.OracleCBF(m, k)
    o.insert(half)
    missing = int((o.query(live) == 0).sum())
    assert 0 < missing < live.size
    before = f.counters()
    assert f.audit(t) == (live.size, missing)
    assert np.array_equal(f.counters(), before)  # the audit changes nothing
    f.rebuild(t)
    assert f.audit(t) == (live.size, 0)
    f.close()
    t.close()


def test_rebuild_and_audit_refuse_bad_arguments():
    L = P.load_library()
    t = P.CCEH(depth=1, max_batch=4096, max_segments=64)
    f = P.CountingBloomFilter(3, 4099)
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert L.pmdfc_cbf_rebuild(None, t.handle, 0, None, None) == -1
    assert L.pmdfc_cbf_rebuild(f._h, None, 0, None, None) == -1
    assert L.pmdfc_cbf_rebuild(f._h, t.handle, 2, None, None) == -1  # an unknown flag
    assert L.pmdfc_cbf_audit(f._h, t.handle, None, None) == -1
    assert L.pmdfc_cbf_audit(None, t.handle, out.data_ptr(), None) == -1
    assert L.pmdfc_cbf_rebuild(f._h, t.handle, 0, None, None) == 0  # the count is optional
    torch.cuda.synchronize()
    assert not f.counters().any()
    f.close()
    t.close()


# ---- 8. the front-end: a warm start admits every restored key

@pytest.mark.parametrize("waves", [1, 8])
def test_kv_load_rebuilds_the_attached_filter(waves, scen, serial, tmp_path):
    init_cap, conv, ops, keys, vals = scen["cap2_ins3k"]
    d0, live, loss = serial["cap2_ins3k"]
    ins = ops == P.OP_INSERT
    m, k = 100003, 5
    want = want_counters(m, k, live)
    path = tmp_path / "table.img"
    kv = KV(init_cap, max_batch=4096, max_segments=1024, serve_waves=waves)
    f1 = P.CountingBloomFilter(k, m)
    kv.attach_counting_bf(f1)
    kv.ops(ops[ins], keys[ins], vals[ins], run=0)  # per op: the serving waves count each Insert
    kv.save(path)
    assert kv.audit_filter() == (live.size, 0)
    assert np.array_equal(f1.counters(), want)
    kv.close()
    kv = KV(init_cap, max_batch=4096, max_segments=1024, serve_waves=waves)
    f2 = P.CountingBloomFilter(k, m)
    kv.attach_counting_bf(f2)
    assert kv.audit_filter() == (0, 0)
    kv.load(path)
    assert np.array_equal(f2.counters(), f1.counters()) and np.array_equal(f2.counters(), want)
    assert np.all(f2.Query(live) == 1) and np.all(f2.QueryBitBloom(live) == 1)  # (Load packs the bitmap too)
    o = O.OracleCBF(m, k)
    o.insert(live)
    assert np.array_equal(f2.bitmap(), o.bitmap())
    assert kv.audit_filter() == (live.size, 0)
    # a refused image (a truncated file) leaves the filter unchanged
    cut = tmp_path / "cut.img"
    cut.write_bytes(path.read_bytes()[:-4096])
    with pytest.raises(P.PmdfcError):
        kv.load(cut)
    assert np.array_equal(f2.counters(), want)
    # the restarted waves count into the rebuilt filter
    more = uniform_keys(4711, 0, 500)
    kv.ops(np.ones(more.size, np.uint8), more, more, run=0)
    o.insert(more)
    assert np.array_equal(f2.counters(), o.counters)
    assert kv.audit_filter() == (live.size + more.size, 0)
    assert kv.rebuild_filter() == live.size + more.size
    assert np.array_equal(f2.counters(), o.counters)
    assert kv.phase()["failed_ops"] == 0
    kv.attach_counting_bf(None)
    with pytest.raises(P.PmdfcError):
        kv.rebuild_filter()
    kv.close()
    f1.close()
    f2.close()


def test_kv_load_without_a_filter_is_the_plain_load(scen, serial, tmp_path):
    init_cap, conv, ops, keys, vals = scen["cap2_ins3k"]
    d0, live, loss = serial["cap2_ins3k"]
    o = O.OracleCCEH(d0)
    o.mixed(ops, keys, vals)
    path = tmp_path / "t.img"
    path.write_bytes(I.image_from_dump(o.dump(), d0))
    kv = KV(init_cap, max_batch=4096, max_segments=1024, serve_waves=1)
    kv.load(path)
    d, od = kv.dump(), o.dump()
    for name in ("dir_canon", "local_depth", "prefix", "keys", "values"):
        assert np.array_equal(d[name], od[name]), name
    with pytest.raises(P.PmdfcError):
        kv.audit_filter()
    kv.close()


def test_facades_rebuild_the_filter_on_load(tmp_path):
    """GpuCCEH : IHash and GpuCCEHHybrid : ICCEH (tests/cpp/test_gpu_filter_kv.cpp,
    a program of its own: the facades are C++)."""
    exe = os.path.join(os.path.dirname(P.engine.LIB_PATH), "test_gpu_filter_kv")
    r = subprocess.run([exe, str(tmp_path), "3000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("GpuCCEH filter_trip_bad 0", "GpuCCEHHybrid filter_trip_bad 0", "filter_kv_bad 0"):
        assert line in r.stdout, r.stdout
