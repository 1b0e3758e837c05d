"""pmdfc_cceh_snapshot_packed, pmdfc_cceh_restore of a packed image and
pmdfc_cceh_export_entries on the GPU.

The packed image is the canonical dump with the empty slots left out, so the
serial oracle says what its bytes must be: packed_from_dump(oracle.dump()).
As in test_gpu_snapshot, snapshot bugs and restore bugs are told apart:
snapshots are compared with the oracle's bytes, restores start from images the
engine never produced.  The rank arithmetic (count, scan, ballot, mbcnt) is
exercised with crafted occupancy patterns; all comparisons are exact.
"""
import ctypes as C
import os
import struct
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
from test_gpu_snapshot import (CUTTINGS, ERR_ARG, ERR_SIZE, IMAGE_NAMES, _default_knobs, _depth, _ring_order,  # noqa: E402,F401
                               _used_engine, code, finals, run, same_answers, same_dump, scen, snap)
from test_packed_image_format import packed_corruptions  # noqa: E402

INVALID, SENTINEL = np.uint64(2**64 - 1), np.uint64(2**64 - 2)
MB, MS = 4096, 4096  # max_batch, max_segments


def psnap(t) -> bytes:
    return t.snapshot(packed=True).cpu().numpy().tobytes()


def live_pairs(d):
    live = d["keys"] != INVALID
    return d["keys"][live], d["values"][live]


def same_items(t, d):
    k, v = t.items()
    wk, wv = live_pairs(d)
    assert k.dtype == torch.int64 and k.is_cuda and v.is_cuda
    assert np.array_equal(k.cpu().numpy().view(np.uint64), wk)
    assert np.array_equal(v.cpu().numpy().view(np.uint64), wv)


# ---- 1. the packed snapshot equals the oracle's bytes

@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_packed_snapshot_equals_oracle_image(name, scen, finals):
    init_cap, conv, ops, keys, vals = scen[name]
    d0, _, od, _ = finals[name]
    want = I.packed_from_dump(od, d0)
    nseg = len(od["local_depth"])
    if name == "src_cap2m_ins50k":  # more segments than one block of the live-count scan takes
        assert nseg > P.load_library().pmdfc_cceh_packed_scan_block() >= 1
    for cut, (max_batch, bounds) in CUTTINGS.items():
        t = P.CCEH(init_cap, convention=conv, max_batch=max_batch or len(ops), max_segments=MS)
        t.MixedBatches(ops, keys, vals, bounds(len(ops)))
        before = t.dump()
        got = psnap(t)
        assert len(got) == len(want) and got == want, (name, cut)
        same_dump(t.dump(), before)  # a snapshot changes nothing
        h = I.validate_packed(got)
        assert h["live"] == live_pairs(od)[0].size and h["nseg"] == nseg
        t.close()


@pytest.mark.parametrize("init_cap", [2, 1024])
def test_packed_snapshot_of_a_fresh_table(init_cap):
    t = P.CCEH(init_cap, max_batch=MB, max_segments=MS)
    d0 = t.initial_depth
    od = O.OracleCCEH(d0).dump()
    want = I.packed_from_dump(od, d0)
    before = t.dump()
    assert psnap(t) == want
    same_dump(t.dump(), before)
    h = I.validate_packed(want)
    assert (h["nseg"], h["live"], h["depth"]) == (1 << d0, 0, d0)
    assert len(want) == I.packed_total_bytes(1 << d0, 0)
    k, v = t.items()
    assert k.numel() == 0 and v.numel() == 0
    t.close()


def test_packed_snapshot_sizing_and_short_buffer(finals):
    d0, _, od, img = finals["cap2_ins3k"]
    want = I.packed_from_dump(od, d0)
    t = P.CCEH(depth=d0, max_batch=MB, max_segments=MS)
    t.restore(img)
    L = P.load_library()
    need, got = C.c_uint64(), C.c_uint64()
    assert L.pmdfc_cceh_snapshot_packed(t.handle, None, 0, C.byref(need), None) == ERR_SIZE
    assert need.value == len(want)
    buf = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    assert L.pmdfc_cceh_snapshot_packed(t.handle, buf.data_ptr(), need.value - 1, C.byref(got), None) == ERR_SIZE
    assert got.value == need.value and not buf.any()  # the exact size, nothing written
    assert L.pmdfc_cceh_snapshot_packed(t.handle, buf.data_ptr() + 8, need.value, C.byref(got), None) == ERR_ARG  # alignment
    assert L.pmdfc_cceh_snapshot_packed(t.handle, buf.data_ptr(), need.value, C.byref(got), None) == 0
    assert buf.cpu().numpy().tobytes() == want
    t.close()


# ---- 2. restore from packed images the engine never produced

@pytest.mark.parametrize("name", IMAGE_NAMES + ["fresh"])
def test_restore_oracle_packed_image(name, scen, finals):
    """The whole stream's table (what test_restore_oracle_image restores)."""
    if name == "fresh":
        d0, conv, keys = 4, "hybrid", uniform_keys(77, 0, 500)
        o = O.OracleCCEH(d0)
        od = o.dump()
        img = I.image_from_dump(od, d0)
    else:
        _, conv, _, keys, _ = scen[name]
        d0, o, od, img = finals[name]
    packed = I.packed_from_dump(od, d0)
    t = P.CCEH(depth=d0, convention=conv, max_batch=MB, max_segments=MS)
    t.restore(packed)
    assert snap(t) == img
    same_dump(t.dump(), od)
    s = t.stats()
    assert s["depth"] == od["depth"] and s["segments"] == len(od["local_depth"]) == o.num_segments
    assert t.Capacity() == o.capacity() and abs(t.Utilization() - o.utilization()) < 1e-9
    assert (s["splits"], s["doublings"], s["split_loss"], s["insert_passes"], s["batches"], s["error_flags"]) == \
        (0, 0, 0, 0, 0, 0)
    q = np.concatenate([keys, uniform_keys(4243, 0, 1000)])
    gv, gs = t.Get(q)
    ov, os_ = o.get(q)
    same_answers(gv, gs, ov, os_)
    fq = S.findany_queries(keys)
    fv, fs = t.FindAnyway(fq)
    ofv, ofs = o.find_anyway(fq)
    same_answers(fv, fs, ofv, ofs)
    assert psnap(t) == packed  # and back out unchanged
    t.close()


@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_stream_continues_after_packed_restore(name, scen):
    """The oracle takes the first half; the engine is restored from the packed
    image of that table and takes the second half op for op like the oracle:
    the later inserts and splits read the occupancy words, local depths and
    directory the restore built."""
    init_cap, conv, ops, keys, vals = scen[name]
    d0 = _depth(init_cap, conv)
    cut = len(ops) // 2
    o = O.OracleCCEH(d0)
    o.mixed(ops[:cut], keys[:cut], vals[:cut])
    od = o.dump()
    t = P.CCEH(init_cap, convention=conv, max_batch=MB, max_segments=MS)
    t.restore(I.packed_from_dump(od, d0))
    assert snap(t) == I.image_from_dump(od, d0)
    same_dump(t.dump(), od)
    out, st = run(t, ops[cut:], keys[cut:], vals[cut:], MB)
    ov, ost = o.mixed(ops[cut:], keys[cut:], vals[cut:])
    same_answers(out, st, ov, ost)
    od = o.dump()
    same_dump(t.dump(), od)
    assert t.stats()["error_flags"] == 0
    assert psnap(t) == I.packed_from_dump(od, d0)
    t.close()


# ---- 3. crafted occupancy: where rank arithmetic breaks

ALL = list(range(1024))
PATTERNS = {
    "slot_0": ([0], [0]),
    "slot_1023": ([1023], [1023]),
    "group_edges": ([63, 64, 255, 256], [63, 64, 255, 256]),
    "odd_slots": (ALL[1::2], ALL[1::2]),
    "all_slots": (ALL, ALL),
    "empty_beside_full": ([], ALL),
    "full_beside_empty": (ALL, []),
    "wave_edges_mixed": ([0, 62, 63, 64, 65, 127, 128, 511, 512, 767, 768, 1022, 1023], ALL[::3]),
}


@pytest.fixture(scope="module")
def keys_by_top_bit():
    k = uniform_keys(20240, 0, 6000)
    top = (O.hash64(k) >> np.uint64(63)).astype(np.int64)
    out = [k[top == 0], k[top == 1]]
    assert min(len(out[0]), len(out[1])) >= 1024
    return out


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_crafted_occupancy(pattern, keys_by_top_bit):
    """Two segments of depth 1, built with numpy; keys go to the segment their
    top hash bit selects."""
    keys = np.full(2048, INVALID, np.uint64)
    for seg, slots in enumerate(PATTERNS[pattern]):
        keys[seg * 1024 + np.asarray(slots, np.int64)] = keys_by_top_bit[seg][:len(slots)]
    vals = np.where(keys != INVALID, keys ^ np.uint64(0x5A5A), np.uint64(0))
    d = {"local_depth": np.array([1, 1], np.uint32), "keys": keys, "values": vals}
    v1, packed = I.image_from_dump(d, 1), I.packed_from_dump(d, 1)
    t = P.CCEH(depth=1, max_batch=MB, max_segments=MS)
    t.restore(packed)
    assert snap(t) == v1
    assert psnap(t) == packed
    same_items(t, d)
    # (the slots are not the keys' probe windows: FindAnyway, which scans the segment)
    fv, _ = t.FindAnyway(keys[keys != INVALID])
    assert np.array_equal(fv, vals[keys != INVALID])
    t.close()


def test_full_parent_of_split_shapes():
    """All 1,024 slots of a segment, reached by inserts: the image part of the
    full_alt stream (tests/golden/split_shapes.json's completely full parent)."""
    init_cap, conv, ops, keys, vals = S.split_shapes(O.hash64)["full_alt"]
    n = S.split_shape_image_size(keys)
    a = P.CCEH(init_cap, convention=conv, max_batch=MB, max_segments=MS)
    for lo in range(0, n, 256):
        a.Insert(keys[lo:lo + 256][:n - lo], vals[lo:lo + 256][:n - lo])
    d = a.dump()
    per_seg = (d["keys"].reshape(-1, 1024) != INVALID).sum(axis=1)
    assert per_seg.max() == 1024  # the premise: a completely full segment
    packed = psnap(a)
    assert packed == I.packed_from_dump(d, a.initial_depth)
    same_items(a, d)
    b = P.CCEH(init_cap, convention=conv, max_batch=MB, max_segments=MS)
    b.restore(packed)
    assert snap(b) == snap(a) and psnap(b) == packed
    same_items(b, d)
    a.close()
    b.close()


# ---- 4. items()

@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_items_are_the_live_pairs_in_order(name, scen, finals):
    init_cap, conv, ops, keys, vals = scen[name]
    d0, _, od, _ = finals[name]
    t = P.CCEH(init_cap, convention=conv, max_batch=MB, max_segments=MS)
    t.MixedBatches(ops, keys, vals, list(range(0, len(ops), MB)) + [len(ops)])
    before = t.dump()
    same_items(t, od)
    L = P.load_library()
    n = C.c_uint64()
    assert L.pmdfc_cceh_export_entries(t.handle, None, None, 0, C.byref(n), None) == ERR_SIZE
    live = I.validate_packed(psnap(t))["live"]
    assert n.value == live == live_pairs(od)[0].size
    if live:
        # too small a capacity: the size again, nothing written; one array alone
        kbuf = torch.zeros(live, dtype=torch.int64, device="cuda")
        n2 = C.c_uint64()
        assert L.pmdfc_cceh_export_entries(t.handle, kbuf.data_ptr(), None, live - 1, C.byref(n2), None) == ERR_SIZE
        assert n2.value == live and not kbuf.any()
        assert L.pmdfc_cceh_export_entries(t.handle, kbuf.data_ptr(), None, live, C.byref(n2), None) == 0
        assert np.array_equal(kbuf.cpu().numpy().view(np.uint64), live_pairs(od)[0])
        vbuf = torch.zeros(live + 3, dtype=torch.int64, device="cuda")
        assert L.pmdfc_cceh_export_entries(t.handle, None, vbuf.data_ptr(), live + 3, C.byref(n2), None) == 0
        got = vbuf.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:live], live_pairs(od)[1]) and not got[live:].any()
    same_dump(t.dump(), before)
    t.close()


# ---- 5. refusals before the table is touched

def test_packed_restore_refusals_leave_the_table(finals):
    d0, o, od, img = finals["cap8_ins20k"]
    packed = I.packed_from_dump(od, d0)
    nseg = len(od["local_depth"])
    t, before = _used_engine(max_segments=256)
    kept = snap(t)
    bad = packed_corruptions(packed, d0)
    assert {"magic", "version", "one_byte_short", "occ_bit_flipped", "live_plus_one", "live_minus_one",
            "header_padding", "depth_padding", "occ_padding", "pair_padding", "below_initial_depth", "depth_31",
            "gap", "overlap"} <= set(bad)
    for case, b in bad.items():
        with pytest.raises(P.PmdfcError) as e:
            t.restore(b)
        assert code(e) == ERR_ARG, case
        assert snap(t) == kept, case
    assert t.stats()["splits"] > 0  # not even the counters were touched
    same_dump(t.dump(), before)
    t.close()
    # more segments than the arena
    t, before = _used_engine(max_segments=nseg - 1)
    kept = snap(t)
    with pytest.raises(P.PmdfcError) as e:
        t.restore(packed)
    assert code(e) == ERR_SIZE
    assert snap(t) == kept
    t.close()
    t, _ = _used_engine(max_segments=nseg)
    t.restore(packed)
    same_dump(t.dump(), od)
    t.close()


def test_packed_restore_refuses_another_shard():
    ld = np.array([3, 4, 4], np.uint32)
    d = {"local_depth": ld, "keys": np.full(3 * 1024, INVALID, np.uint64), "values": np.zeros(3 * 1024, np.uint64)}
    packed = I.packed_from_dump(d, 3, shard_bits=2, shard_id=3)
    k = uniform_keys(5, 0, 8000)
    for kw, ok in ((dict(depth=3, shard_bits=2, shard_id=2), False), (dict(depth=4, shard_bits=2, shard_id=3), False),
                   (dict(depth=3, shard_bits=0, shard_id=0), False), (dict(depth=3, shard_bits=2, shard_id=3), True)):
        t = P.CCEH(max_batch=MB, max_segments=256, **kw)
        own = k[(P.hash64(k) >> np.uint64(64 - kw["shard_bits"])).astype(np.int64) == kw["shard_id"]] \
            if kw["shard_bits"] else k
        t.Insert(own[:1500], own[:1500])
        kept = snap(t)
        if ok:
            t.restore(packed)
            assert snap(t) == I.unpack(packed) and psnap(t) == packed
        else:
            with pytest.raises(P.PmdfcError) as e:
                t.restore(packed)
            assert code(e) == ERR_ARG
            assert snap(t) == kept
        t.close()


# ---- 6. refusals after the device pass

def test_packed_restore_refuses_bad_stored_keys(finals):
    """A dense pair whose key is INVALID or SENTINEL, and two keys exchanged
    between segments of different prefix, pass every host check (the occupancy
    words still count `live`); the device pass counts them and the table is
    left freshly reset."""
    d0, o, od, img = finals["cap8_ins20k"]
    packed = np.frombuffer(I.packed_from_dump(od, d0), np.uint8)
    nseg = len(od["local_depth"])
    p = I.packed_pairs_offset(nseg)
    per_seg = (od["keys"].reshape(nseg, 1024) != INVALID).sum(axis=1)
    assert per_seg[0] > 5 and per_seg[-1] > 0
    first_of_last = int(per_seg[:-1].sum())

    def edited(f):
        b = packed.copy()
        f(b[p:p + int(per_seg.sum()) * 16].view(np.uint64).reshape(-1, 2))
        I.validate_packed(b)  # nothing the host can see
        return b

    def swap(pairs):
        pairs[[0, first_of_last]] = pairs[[first_of_last, 0]]

    cases = {
        "invalid": edited(lambda pairs: pairs.__setitem__((first_of_last, 0), INVALID)),
        "sentinel": edited(lambda pairs: pairs.__setitem__((5, 0), SENTINEL)),
        "moved": edited(swap),
    }
    fresh = P.CCEH(8, max_batch=MB, max_segments=256)
    want = fresh.dump()
    fresh.close()
    for case, b in cases.items():
        t, _ = _used_engine(max_segments=256)
        with pytest.raises(P.PmdfcError) as e:
            t.restore(b)
        assert code(e) == ERR_ARG, case
        same_dump(t.dump(), want)
        s = t.stats()
        assert s["segments"] == 8 and s["splits"] == 0 and s["error_flags"] == 0
        k = uniform_keys(98, 0, 3000)  # and it works on from there
        o2 = O.OracleCCEH(3)
        assert np.array_equal(t.Insert(k, k), o2.insert(k, k))
        same_dump(t.dump(), o2.dump())
        t.close()


# ---- 7. files and the front-end

def test_cceh_save_packed_and_load(finals, tmp_path):
    d0, o, od, img = finals["cap8_ins20k"]
    packed = I.packed_from_dump(od, d0)
    t = P.CCEH(depth=d0, max_batch=MB, max_segments=MS)
    t.restore(img)
    pp, pv = tmp_path / "t.pak", tmp_path / "t.img"
    assert t.save(pp, packed=True) == len(packed) and t.save(pv) == len(img)
    assert pp.read_bytes() == packed and pv.read_bytes() == img
    # smaller by exactly the empty slots, less the occupancy words: from the header
    raw = pp.read_bytes()[:64]
    nseg, live, total = struct.unpack("<3Q", raw[40:64])
    occ_bytes = (nseg * 128 + 4095) // 4096 * 4096
    pair_bytes = (live * 16 + 4095) // 4096 * 4096
    assert total == os.path.getsize(pp)
    assert os.path.getsize(pv) - os.path.getsize(pp) == nseg * 16384 - (occ_bytes + pair_bytes) > 0
    u = P.CCEH(depth=d0, max_batch=500, max_segments=MS)
    u.load(pp)
    same_dump(u.dump(), od)
    assert snap(u) == img
    t.close()
    u.close()


@pytest.mark.parametrize("waves", [1, 8])
def test_kv_save_packed_load_through_the_rings(waves, scen, tmp_path):
    init_cap, conv, ops, keys, vals = scen["mixed_cap2_30k_ins80"]
    half = len(ops) // 2
    path = tmp_path / "table.pak"
    o = O.OracleCCEH(1)
    kv = KV(init_cap, max_batch=MB, max_segments=MS, serve_waves=waves)
    f1 = P.CountingBloomFilter(4, 1 << 20)
    kv.attach_counting_bf(f1)
    vo, st, pl = kv.ops(ops[:half], keys[:half], vals[:half], run=0)
    order = _ring_order(pl)
    ov, ost = o.mixed(ops[:half][order], keys[:half][order], vals[:half][order])
    same_answers(vo[order], st[order], ov, ost)
    kv.save(path, packed=True)
    od = o.dump()
    assert path.read_bytes() == I.packed_from_dump(od, 1)
    live = live_pairs(od)[0].size
    assert kv.phase()["failed_ops"] == 0
    kv.close()
    kv = KV(init_cap, max_batch=MB, max_segments=MS, serve_waves=waves)
    f2 = P.CountingBloomFilter(4, 1 << 20)
    kv.attach_counting_bf(f2)
    kv.load(path)
    same_dump(kv.dump(), od)
    assert kv.audit_filter() == (live, 0)  # the filter rebuilt from the loaded table: no stored key missing
    vo, st, pl = kv.ops(ops[half:], keys[half:], vals[half:], run=0)
    order = _ring_order(pl)
    ov, ost = o.mixed(ops[half:][order], keys[half:][order], vals[half:][order])
    same_answers(vo[order], st[order], ov, ost)
    same_dump(kv.dump(), o.dump())
    assert kv.audit_filter()[1] == 0
    ph = kv.phase()
    assert ph["failed_ops"] == 0 and kv.stats()["error_flags"] == 0
    cut = tmp_path / "cut.pak"
    cut.write_bytes(path.read_bytes()[:-1])
    with pytest.raises(P.PmdfcError):
        kv.load(cut)
    same_dump(kv.dump(), o.dump())
    kv.close()
    f1.close()
    f2.close()


def test_facades_save_packed_and_load(tmp_path):
    """GpuCCEH : IHash and GpuCCEHHybrid : ICCEH (tests/cpp/test_gpu_packed_kv.cpp,
    a program of its own: the facades are C++)."""
    exe = os.path.join(os.path.dirname(P.engine.LIB_PATH), "test_gpu_packed_kv")
    r = subprocess.run([exe, str(tmp_path), "6000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("GpuCCEH packed_round_trip_bad 0", "GpuCCEHHybrid packed_round_trip_bad 0",
                 "packed_cross_load_bad 0", "packed_kv_bad 0"):
        assert line in r.stdout, r.stdout
