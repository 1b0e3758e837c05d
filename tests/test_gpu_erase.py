"""pmdfc_cceh_erase on the GPU: batched key removal that keeps
the probe invariant.

There is no reference implementation of Erase; the contract is the serial
rule, and tests/erase_ref.py models it.  Every comparison here is against that
model applied to the dump the engine gave BEFORE the erase, and after each
case limits_ref.check_table runs on the engine's dump (its last assertion is
Invariant I: no empty slot between a stored key's window start and the key).
"""
import os
import subprocess

import numpy as np
import pytest

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
CUTS = [1, 23, 64, 65, 1000, 0]  # erases per batch; 0: the whole plan as one batch
MAX_SEGS = 256


@pytest.fixture(scope="module")
def scen():
    s = S.scenarios(O.hash64)
    s.update(S.upsert_scenarios(O.hash64))
    return s


def dev(keys):
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).cuda()


def filled(stream, upsert=False, max_batch=16384):
    init_cap, conv, ops, keys, vals = stream
    t = P.CCEH(init_cap, convention=conv, max_batch=max_batch, max_segments=MAX_SEGS, upsert=upsert)
    for lo in range(0, len(ops), 4096):
        t.Mixed(ops[lo:lo + 4096], keys[lo:lo + 4096], vals[lo:lo + 4096])
    return t


def erase_cut(t, plan, cut):
    k = dev(plan)
    if cut == 0:
        return t.Erase(k).cpu().numpy()
    return torch.cat([t.Erase(k[lo:lo + cut]) for lo in range(0, k.numel(), cut)]).cpu().numpy()


def checked_dump(t, max_segments=MAX_SEGS):
    d = t.dump()
    s = t.stats()
    R.check_table(d, s, max_segments)
    assert s["error_flags"] == 0
    return d


_MODELLED = {}


def modelled(name, pre, ins_keys, upsert=False):
    """The plan of a stream and the model's answer to it, computed once from
    the first dump taken before an erase; every later case must start from
    the same table."""
    if name not in _MODELLED:
        plan, stay = E.erase_plan(ins_keys, 77)
        m = E.ErasableTable(pre, upsert=upsert)
        st = m.erase_batch(plan)
        _MODELLED[name] = (pre, plan, stay, st, m.image(), m.live(), (m.moves, m.max_chain))
    assert R.same_image(pre, _MODELLED[name][0]), "the table before the erase differs between cases"
    return _MODELLED[name][1:]


# ---- 1. the fixture streams, every cutting

def _stream_case(scen, name, cut, upsert=False):
    stream = scen[name]
    ops, keys = stream[2], stream[3]
    t = filled(stream, upsert=upsert)
    pre = checked_dump(t)
    plan, stay, want_st, want_img, want_live, chains = modelled(name, pre, keys[np.asarray(ops) == P.OP_INSERT], upsert)
    st = erase_cut(t, plan, cut)
    assert np.array_equal(st, want_st), (name, cut, np.nonzero(st != want_st)[0][:10])
    assert np.count_nonzero(st == P.ST_ERASED) > 100 and np.count_nonzero(st == P.ST_MISS) > 100
    assert np.count_nonzero(st == P.ST_RESERVED_KEY) == 2
    d = checked_dump(t)
    assert R.same_image(d, want_img), (name, cut)  # the model's: so every cutting gives the same dump
    assert t.items()[0].numel() == want_live
    if cut == 0:
        print(f"{name}: {plan.size} erases, {np.count_nonzero(st == P.ST_ERASED)} ERASED, "
              f"{chains[0]} entries moved, longest chain {chains[1]}")
    return t, plan, stay, st


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("name", STREAMS)
def test_stream_erase_equals_model(scen, name, cut):
    t, *_ = _stream_case(scen, name, cut)
    t.close()


# ---- 2. batch order

def test_batch_order_statuses(scen):
    """One batch: a stored key three times, an absent key twice, a key stored 32 times."""
    stream = scen["dup32"]
    t = filled(stream)
    pre = checked_dump(t)
    m = E.ErasableTable(pre)
    ins = stream[3][np.asarray(stream[2]) == P.OP_INSERT]
    u, c = np.unique(ins, return_counts=True)
    k32, k1, absent = int(u[np.argmax(c)]), int(u[c == 1][0]), 0x123456789ABCDEF
    assert len(m.copies(k32)) == 32 and m.get(absent)[1] == R.ST_MISS
    batch = np.array([k1, k1, k1, absent, absent, k32], np.uint64)
    st = t.Erase(batch)
    assert st.tolist() == [P.ST_ERASED, P.ST_MISS, P.ST_MISS, P.ST_MISS, P.ST_MISS, P.ST_ERASED]
    assert np.array_equal(st, m.erase_batch(batch))
    assert R.same_image(checked_dump(t), m.image())
    v, gs = t.Get(batch)
    assert np.all(gs == P.ST_MISS) and np.all(v == 0)
    # a batch that is one stored key many times: one wave, one run
    k2 = int(u[c == 1][1])
    st = t.Erase(np.full(500, k2, np.uint64))
    assert st.tolist() == [P.ST_ERASED] + [P.ST_MISS] * 499
    assert np.array_equal(st, m.erase_batch(np.full(500, k2, np.uint64)))
    assert R.same_image(checked_dump(t), m.image())
    assert t.Erase(np.zeros(0, np.uint64)).size == 0
    # n > max_batch: the binding cuts long inputs, the C call refuses them
    k = dev(np.zeros(t.max_batch + 1, np.uint64))
    s = torch.empty(k.numel(), dtype=torch.uint8, device="cuda")
    assert P.load_library().pmdfc_cceh_erase(t.handle, k.data_ptr(), s.data_ptr(), k.numel(), None) == -1  # PMDFC_ERR_ARG
    t.close()


def test_wrong_shard_is_gets_answer():
    keys = uniform_keys(41, 0, 4000)
    t = P.CCEH(depth=3, shard_bits=1, shard_id=1, max_batch=4096, max_segments=64)
    ist = t.Insert(keys, keys)
    _, gst = t.Get(keys)
    assert np.count_nonzero(gst == P.ST_WRONG_SHARD) > 1000 and np.count_nonzero(gst == P.ST_HIT) > 1000
    est = t.Erase(keys)
    assert np.array_equal(est == P.ST_WRONG_SHARD, gst == P.ST_WRONG_SHARD)
    assert np.array_equal(est == P.ST_ERASED, ist == P.ST_INSERTED)
    _, gst = t.Get(keys)
    assert np.all((gst == P.ST_WRONG_SHARD) | (gst == P.ST_MISS))
    assert t.items()[0].numel() == 0 and t.stats()["error_flags"] == 0
    t.close()


# ---- 3. long chains and the wrap: the crafted images of scenarios.split_shapes

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


def _target_rows(d, prefix, L):
    seg = int(np.nonzero((np.asarray(d["local_depth"]) == L) & (np.asarray(d["prefix"]) == prefix))[0][0])
    return np.asarray(d["keys"], np.uint64).reshape(-1, 1024)[seg]


def test_long_chain_backlog():
    """backlog_c0: one 628-slot cluster from slot 200 on.  The entry at the
    cluster's first slot goes, then whatever stands in the first line, one
    erase at a time: every removal pulls a chain through the cluster."""
    t, pre, prefix, L = shape_table("backlog_c0")
    m = E.ErasableTable(pre)
    row = _target_rows(pre, prefix, L)
    assert np.all(row[200:828] != np.uint64(R.INVALID)) and row[199] == row[828] == np.uint64(R.INVALID)
    for i in range(12):
        k = int(_target_rows(m.image(), prefix, L)[200 + i % 4])
        assert k != R.INVALID
        assert t.Erase(np.array([k], np.uint64)).tolist() == [m.erase(k)] == [P.ST_ERASED]
        assert R.same_image(checked_dump(t, 64), m.image()), i
    assert m.max_chain >= 100  # (the chains are long: what the case is for)
    print(f"backlog_c0: {m.moves} entries moved by 12 erases, longest chain {m.max_chain}")
    t.close()


def test_full_segment_erase_then_refill():
    """full_alt: all 1,024 slots taken.  64 seeded keys go; 64 fresh keys of
    the same segment and home lines are INSERTED into the freed slots with no
    split."""
    t, pre, prefix, L = shape_table("full_alt")
    m = E.ErasableTable(pre)
    row = _target_rows(pre, prefix, L)
    assert np.all(row != np.uint64(R.INVALID))
    gone = row[np.random.default_rng(31).permutation(1024)[:64]]
    assert np.array_equal(t.Erase(gone), m.erase_batch(gone))
    assert R.same_image(checked_dump(t, 64), m.image())
    lines = (O.hash64(gone) & np.uint64(0xFF)).tolist()
    fresh = np.concatenate([S.keys_from_hash_fields(prefix, L, ln, 1, first=(1 << 30) + i) for i, ln in enumerate(lines)])
    assert not np.any(np.isin(fresh, row))
    splits = t.stats()["splits"]
    st = t.Insert(fresh, fresh ^ np.uint64(3))
    assert np.all(st == P.ST_INSERTED) and np.array_equal(st, m.insert_batch(fresh, fresh ^ np.uint64(3)))
    assert t.stats()["splits"] == splits and t.stats()["segments"] == len(pre["local_depth"])
    d = checked_dump(t, 64)
    assert R.same_image(d, m.image())
    assert np.all(_target_rows(d, prefix, L) != np.uint64(R.INVALID))  # full again
    t.close()


@pytest.mark.parametrize("name", ["wide_wrap", "cyclic_heads"])
def test_shifts_across_the_wrap(name):
    """The keys whose home line is >= 249 (their windows reach past slot 1023) go: the shifts cross the wrap."""
    t, pre, prefix, L = shape_table(name)
    m = E.ErasableTable(pre)
    row = _target_rows(pre, prefix, L)
    row = row[row != np.uint64(R.INVALID)]
    gone = row[(O.hash64(row) & np.uint64(0xFF)) >= np.uint64(249)]
    assert gone.size >= 20
    gone = gone[np.random.default_rng(32).permutation(gone.size)]
    st = t.Erase(gone)
    assert np.all(st == P.ST_ERASED) and np.array_equal(st, m.erase_batch(gone))
    assert R.same_image(checked_dump(t, 64), m.image())
    v, gs = t.Get(row)
    mv = [m.get(int(k)) for k in row.tolist()]
    assert v.tolist() == [x[0] for x in mv] and gs.tolist() == [x[1] for x in mv]
    print(f"{name}: {gone.size} erases, {m.moves} entries moved, longest chain {m.max_chain}")
    t.close()


# ---- 4. no hidden state

def test_no_hidden_state_after_erase():
    """Engine A inserts, erases and inserts on (splitting and doubling); engine
    B starts from the image of the MODEL's table after the erase and gets the
    same inserts: the same statuses and the same final table."""
    keys = uniform_keys(51, 0, 20000)
    a = P.CCEH(depth=3, max_batch=16384, max_segments=512)
    assert np.all(a.Insert(keys, keys ^ np.uint64(9)) == P.ST_INSERTED)
    pre = checked_dump(a, 512)
    m = E.ErasableTable(pre)
    gone = keys[np.random.default_rng(52).random(keys.size) < 0.5]
    assert np.array_equal(a.Erase(gone), m.erase_batch(gone))
    assert R.same_image(checked_dump(a, 512), m.image())
    packed = a.snapshot(packed=True).cpu().numpy().tobytes()  # PMDFC_ERR_STATE if keys and occupancy words disagree
    assert I.validate_packed(packed)["live"] == m.live() == keys.size - gone.size
    b = P.CCEH(depth=3, max_batch=16384, max_segments=512)
    b.restore(I.image_from_dump(m.image(), 3))
    fresh = uniform_keys(53, 0, 3 * gone.size)
    sa, sb = a.stats(), b.stats()
    for lo in range(0, fresh.size, 8192):
        ka = fresh[lo:lo + 8192]
        assert np.array_equal(a.Insert(ka, ka ^ np.uint64(5)), b.Insert(ka, ka ^ np.uint64(5)))
    da, db = checked_dump(a, 512), checked_dump(b, 512)
    assert R.same_image(da, db)
    assert a.stats()["splits"] > sa["splits"] and a.stats()["segments"] > sa["segments"]
    assert a.stats()["depth"] > sa["depth"]  # it split and doubled
    assert a.stats()["segments"] - sa["segments"] == b.stats()["segments"] - sb["segments"]
    a.close()
    b.close()


# ---- 5. every read path after an erase

def test_read_paths_after_erase():
    keys = uniform_keys(61, 0, 20000)
    t = P.CCEH(depth=4, max_batch=32768, max_segments=512)
    assert np.all(t.Insert(keys, keys ^ np.uint64(0x77)) == P.ST_INSERTED)
    pre = checked_dump(t, 512)
    m = E.ErasableTable(pre)
    rng = np.random.default_rng(62)
    gone = keys[rng.random(keys.size) < 0.5]
    assert np.array_equal(t.Erase(gone), m.erase_batch(gone))
    q = np.concatenate([keys, uniform_keys(63, 0, 1000), np.array([R.INVALID, R.SENTINEL], np.uint64)])
    q = q[rng.permutation(q.size)]
    want = [m.get(int(k)) for k in q.tolist()]
    wv, ws = np.array([x[0] for x in want], np.uint64), np.array([x[1] for x in want], np.uint8)
    assert np.count_nonzero(ws == R.ST_HIT) == keys.size - gone.size
    v, s = t.Get(q)
    assert np.array_equal(v, wv) and np.array_equal(s, ws)
    v, s = t.GetBatches(q, [0, 1, 65, 4096, 4097, q.size])
    assert np.array_equal(v, wv) and np.array_equal(s, ws)
    live = ws < R.ST_RESERVED_KEY  # (FindAnyway takes no reserved key apart; the table is duplicate-free, so its copy is Get's)
    v, s = t.FindAnyway(q[live][:3000])
    assert np.array_equal(v, wv[live][:3000]) and np.array_equal(s, ws[live][:3000])
    # mixed batches on every path: one wave, small, medium, general.  A tenth of
    # the ops insert fresh keys -- too few to fill a window, which the model
    # confirms by answering no CAPACITY -- so nothing splits
    nseg = t.stats()["segments"]
    pos = 0
    for n in (64, 256, 8192, 20000):
        ops = (rng.random(n) < 0.1).astype(np.uint8)
        fresh = uniform_keys(64, pos, n)
        pos += n
        mk = np.where(ops == 1, fresh, keys[rng.integers(0, keys.size, n)])
        again = np.nonzero(ops == 0)[0][::3]  # a third of the Gets ask for erased keys
        mk[again] = gone[rng.integers(0, gone.size, again.size)]
        mv = mk ^ np.uint64(n)
        wv, ws = m.mixed(ops, mk, mv)
        assert not np.any(ws == R.ST_CAPACITY), n  # (a failure, not a skip: the batch must be modelled)
        assert np.all(ws[ops == 1] == R.ST_INSERTED)
        v, s = t.Mixed(ops, mk, mv)
        assert np.array_equal(s, ws) and np.array_equal(v, wv), n
        assert t.stats()["segments"] == nseg
    assert R.same_image(checked_dump(t, 512), m.image())
    t.close()


# ---- 6. churn

def test_churn_rounds():
    """8 rounds over a live set of 32K keys: a seeded half goes, as many fresh
    keys come.  The segment count per round is reported, not bounded: first-fit
    placement in a new order may split where the old order did not."""
    n = 1 << 15
    t = P.CCEH(depth=5, max_batch=n, max_segments=1024)
    rng = np.random.default_rng(71)
    live = uniform_keys(72, 0, n)
    vals = live ^ np.uint64(0xC0FFEE)
    assert np.all(t.Insert(live, vals) == P.ST_INSERTED)
    want = dict(zip(live.tolist(), vals.tolist()))
    pos, segs = n, []
    for r in range(8):
        go = rng.random(live.size) < 0.5
        gone = live[go]
        assert np.all(t.Erase(gone) == P.ST_ERASED)
        for k in gone.tolist():
            del want[k]
        fresh = uniform_keys(72, pos, gone.size)
        pos += gone.size
        fv = fresh ^ np.uint64(r + 1)
        assert np.all(t.Insert(fresh, fv) == P.ST_INSERTED)
        want.update(zip(fresh.tolist(), fv.tolist()))
        live = np.concatenate([live[~go], fresh])
        q = np.concatenate([live, gone])
        v, s = t.Get(q)
        wv = np.array([want.get(k, 0) for k in q.tolist()], np.uint64)
        assert np.array_equal(v, wv) and np.all(s[:live.size] == P.ST_HIT) and np.all(s[live.size:] == P.ST_MISS), r
        assert t.items()[0].numel() == len(want) == n
        st = t.stats()
        assert st["split_loss"] == 0 and st["error_flags"] == 0
        segs.append(st["segments"])
    checked_dump(t, 1024)
    print(f"churn: segments per round {segs}, utilization {t.Utilization():.1f}%")
    t.close()


# ---- 7. upsert mode

@pytest.mark.parametrize("cut", [23, 0])
def test_upsert_stream_and_reinsert(scen, cut):
    t, plan, stay, st = _stream_case(scen, UPSERT_STREAM, cut, upsert=True)
    back = plan[st == P.ST_ERASED][:500]
    twice = np.concatenate([back, back])  # an erased key inserted again: INSERTED, and only then UPDATED
    ist = t.Insert(twice, twice ^ np.uint64(1))
    assert np.all(ist[:back.size] == P.ST_INSERTED) and np.all(ist[back.size:] == P.ST_UPDATED)
    v, s = t.Get(back)
    assert np.all(s == P.ST_HIT) and np.array_equal(v, back ^ np.uint64(1))
    checked_dump(t)
    t.close()


# ---- 8. the counting filter and the front-end

def test_filter_follows_erase_run():
    m_bits, k_hash = 100003, 5
    keys = uniform_keys(81, 0, 6000)
    kv = KV(depth=3, max_batch=2048, max_segments=256, serve_waves=8)  # (the run takes two engine batches)
    f = P.CountingBloomFilter(k_hash, m_bits)
    kv.attach_counting_bf(f)
    _, st, _ = kv.ops(np.ones(keys.size, np.uint8), keys, keys ^ np.uint64(2), run=500)
    assert np.all(st == P.ST_INSERTED)
    gone = keys[np.random.default_rng(82).random(keys.size) < 0.5]
    run = np.concatenate([gone, uniform_keys(83, 0, 100), gone[:50]])  # absent keys and repeats leave the filter alone
    est = kv.erase_run(run)
    assert np.all(est[:gone.size] == P.ST_ERASED) and np.all(est[gone.size:] == P.ST_MISS)
    o = O.OracleCBF(m_bits, k_hash)
    o.insert(keys)
    assert np.all(o.delete(gone) == 1)
    assert np.array_equal(f.counters(), o.counters)
    assert kv.audit_filter() == (keys.size - gone.size, 0)
    vo, st, _ = kv.ops(np.zeros(keys.size, np.uint8), keys, keys, run=500)  # the waves serve again
    was_gone = np.isin(keys, gone)
    assert np.all(st[was_gone] == P.ST_MISS) and np.all(st[~was_gone] == P.ST_HIT)
    assert np.array_equal(vo[~was_gone], keys[~was_gone] ^ np.uint64(2))
    assert kv.stats()["error_flags"] == 0 and kv.phase()["failed_ops"] == 0
    d = kv.dump()
    R.check_table(d, kv.stats(), 256)
    kv.attach_counting_bf(None)
    kv.close()
    f.close()


def test_front_end_erase_between_served_ops():
    """KV.erase one op at a time between served Inserts and Gets, one caller
    thread, 8 waves: every result is a dict's, and the ops after an erase are
    answered (the waves start again)."""
    kv = KV(depth=3, max_batch=4096, max_segments=256, serve_waves=8)
    rng = np.random.default_rng(91)
    pool = uniform_keys(92, 0, 200)
    want = {}
    erased, starts, stopped = 0, 0, True
    for i in range(600):
        k = int(pool[rng.integers(0, pool.size)])
        r = rng.random()
        if r < 0.45:
            if k in want:  # (the table keeps duplicates: insert a key only while it is absent)
                continue
            assert kv.Insert(k, i + 1) == P.ST_INSERTED
            want[k] = i + 1
        elif r < 0.85:
            assert kv.Get(k) == want.get(k, 0)
        else:
            assert kv.erase(k) == (P.ST_ERASED if k in want else P.ST_MISS)
            erased += k in want
            want.pop(k, None)
            stopped = True
            continue
        starts += stopped  # a served op after an erase: the waves had to start again
        stopped = False
    assert erased > 20 and starts > 20
    assert kv.erase(2**64 - 1) == P.ST_RESERVED_KEY
    for k in pool.tolist():
        assert kv.Get(k) == want.get(k, 0)
    ph = kv.phase()
    assert ph["failed_ops"] == 0 and ph["wave_starts"] >= starts  # stopped for every erase, started again
    R.check_table(kv.dump(), kv.stats(), 256)
    kv.close()


def test_facades_erase():
    """GpuCCEH : IHash and GpuCCEHHybrid : ICCEH (tests/cpp/test_gpu_erase_kv.cpp,
    a program of its own: the facades are C++): Erase, EraseBatch, Delete still
    the stub, Erase refused from a completion callback."""
    exe = os.path.join(os.path.dirname(P.engine.LIB_PATH), "test_gpu_erase_kv")
    r = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("GpuCCEH Delete 0", "GpuCCEHHybrid Delete 0", "GpuCCEH callback_bad 0", "GpuCCEHHybrid callback_bad 0",
                 "GpuCCEH erase_trip_bad 0", "GpuCCEHHybrid erase_trip_bad 0", "erase_kv_bad 0"):
        assert line in r.stdout, r.stdout
