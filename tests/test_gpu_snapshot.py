"""pmdfc_cceh_snapshot / pmdfc_cceh_restore on the GPU.

The image is the canonical dump and nothing else, so the serial oracle says
what its bytes must be: image_from_dump(oracle.dump()).  Snapshot bugs and
restore bugs are told apart: snapshots are compared with the oracle's bytes,
restores start from images the engine never produced, and a restored table
then has to behave like the source -- its occupancy words and directory are
only visible in what later inserts, splits and rebuckets do with them.
"""
import contextlib
import ctypes as C
import json
import os
import re
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
from test_gpu_split_shapes import CUTS, _check_ops, _check_table, _classes, _kernel  # noqa: E402
from test_image_format import corruptions  # noqa: E402

ERR_ARG, ERR_SIZE = -1, -5
TIGHT = {"PMDFC_P1MAX": "1", "PMDFC_CHUNK": "61", "PMDFC_FLAT_MAX": "3"}
IMAGE_NAMES = ["cap2_ins3k", "cap8_ins20k", "mixed_cap2_30k_ins80", "dup_wrap", "dup32", "split_loss",
               "split_loss_mixed", "src_cap2m_ins50k"]


@contextlib.contextmanager
def knobs(env):
    """The create-time knobs (knobs.h CreateKnobs) for the engines made inside."""
    old = {k: os.environ.get(k) for k in TIGHT}
    for k in TIGHT:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(autouse=True)
def _default_knobs():
    with knobs({}):
        yield


@pytest.fixture(scope="module")
def scen():
    return S.scenarios(O.hash64)


def _depth(init_cap, conv):
    return O.OracleCCEH.depth_for_hybrid(init_cap) if conv == "hybrid" else O.OracleCCEH.depth_for_src(init_cap)


@pytest.fixture(scope="module")
def finals(scen):
    """name -> (initial depth, the oracle after the whole stream, its dump, its
    image), computed once and left unchanged."""
    out = {}
    for name in IMAGE_NAMES:
        init_cap, conv, ops, keys, vals = scen[name]
        d0 = _depth(init_cap, conv)
        o = O.OracleCCEH(d0)
        o.mixed(ops, keys, vals)
        od = o.dump()
        out[name] = (d0, o, od, I.image_from_dump(od, d0))
    return out


def snap(t) -> bytes:
    return t.snapshot().cpu().numpy().tobytes()


def run(t, ops, keys, vals, batch):
    """The stream through Mixed in batches of `batch` ops (one call per batch)."""
    n = len(ops)
    out, st = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    for lo in range(0, n, batch):
        out[lo:lo + batch], st[lo:lo + batch] = t.Mixed(ops[lo:lo + batch], keys[lo:lo + batch], vals[lo:lo + batch])
    return out, st


def same_dump(d, od):
    assert d["depth"] == od["depth"]
    for f in ("dir_canon", "local_depth", "prefix", "keys", "values"):
        assert np.array_equal(d[f], od[f]), f


def same_answers(out, st, ov, ost):
    bad = np.nonzero((st != ost) | (out != ov))[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], ost[bad[:8]], out[bad[:8]], ov[bad[:8]])


def code(excinfo) -> int:
    return int(re.search(r"failed \((-?\d+)\)", str(excinfo.value)).group(1))


# ---- 1. the image equals the oracle's, byte for byte

# cutting -> (max_batch, the batch bounds of an n-op stream)
CUTTINGS = {
    # one op per batch (k_mixed_tiny) while that stays quick, then 61-op batches
    "one_op": (4096, lambda n: list(range(0, min(n, 3000))) + list(range(min(n, 3000), n, 61)) + [n]),
    "256_op": (4096, lambda n: list(range(0, n, 256)) + [n]),
    "one_batch": (None, lambda n: [0, n]),  # max_batch = n: another p1max, other arena ids and pool offsets
}


@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_snapshot_equals_oracle_image(name, scen, finals):
    init_cap, conv, ops, keys, vals = scen[name]
    d0, _, od, want = finals[name]
    for cut, (max_batch, bounds) in CUTTINGS.items():
        t = P.CCEH(init_cap, convention=conv, max_batch=max_batch or len(ops), max_segments=4096)
        t.MixedBatches(ops, keys, vals, bounds(len(ops)))
        before = t.dump()
        got = snap(t)
        assert len(got) == len(want) and got == want, (name, cut)
        same_dump(t.dump(), before)  # a snapshot changes nothing
        h = I.validate(got)
        assert h["live"] == int((od["keys"] != np.uint64(2**64 - 1)).sum()) and h["nseg"] == len(od["local_depth"])
        t.close()


@pytest.mark.parametrize("init_cap", [2, 1024])
def test_snapshot_of_a_fresh_table(init_cap):
    t = P.CCEH(init_cap, max_batch=4096, max_segments=2048)
    d0 = t.initial_depth
    want = I.image_from_dump(O.OracleCCEH(d0).dump(), d0)
    assert snap(t) == want
    h = I.validate(want)
    assert (h["nseg"], h["live"], h["depth"], h["min_ld"], h["max_ld"]) == (1 << d0, 0, d0, d0, d0)
    t.close()


# ---- 2. restore from an image the engine never produced

@pytest.mark.parametrize("name", IMAGE_NAMES + ["fresh"])
def test_restore_oracle_image(name, scen, finals):
    if name == "fresh":
        d0, conv, keys = 4, "hybrid", uniform_keys(77, 0, 500)
        o = O.OracleCCEH(d0)
        od = o.dump()
        img = I.image_from_dump(od, d0)
    else:
        _, conv, _, keys, _ = scen[name]
        d0, o, od, img = finals[name]
    t = P.CCEH(depth=d0, convention=conv, max_batch=4096, max_segments=4096)
    t.restore(img)
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
    assert snap(t) == img  # and back out unchanged
    t.close()


# ---- 3. continue after restore: occupancy words and directory

@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "split_shapes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def shapes():
    return S.split_shapes(O.hash64)


@pytest.fixture(scope="module")
def serial(shapes):
    out = {}
    for name, (init_cap, conv, ops, keys, vals) in shapes.items():
        o = O.OracleCCEH(O.OracleCCEH.depth_for_hybrid(init_cap))
        ov, ost = o.mixed(ops, keys, vals)
        out[name] = (ov, ost, o.dump(), o.stats()["split_loss"])
    return out


@pytest.fixture(scope="module")
def shape_images(shapes):
    """name -> (the image part's insert statuses, the snapshot of the engine
    that took it), one source engine per shape."""
    out = {}
    for name, (init_cap, conv, ops, keys, vals) in shapes.items():
        n = S.split_shape_image_size(keys)
        a = P.CCEH(init_cap, convention=conv, max_batch=4096, max_segments=64)
        st = np.concatenate([a.Insert(keys[lo:lo + 256][:n - lo], vals[lo:lo + 256][:n - lo])
                             for lo in range(0, n, 256)])
        out[name] = (st, snap(a))
        a.close()
    return out


@pytest.mark.parametrize("cut", list(CUTS))
@pytest.mark.parametrize("name", [b + s for s in S.SPLIT_SHAPE_TABLES for b in S.SPLIT_SHAPES])
def test_split_shape_continues_after_restore(name, cut, shapes, shape_images, golden, serial):
    """The crafted image goes into A; B is restored from A's snapshot and takes
    the rest of the stream: Gets of the image, the trigger insert whose full
    window splits the restored parent, the Gets again, absent keys.  The
    split reads the occupancy words the restore built from the keys."""
    max_batch, before, after, kernel, is_tight = CUTS[cut]
    init_cap, conv, ops, keys, vals = shapes[name]
    n = S.split_shape_image_size(keys)
    st_img, img = shape_images[name]
    if cut == "tight_general":  # pad the rest of the stream past k_medium's 8192 ops with Gets of absent keys
        pad = uniform_keys(902, 0, 8193 - (keys.size - n) + 1000)
        keys = np.concatenate([keys, pad])
        ops = np.concatenate([ops, np.zeros(pad.size, np.uint8)])
        vals = np.concatenate([vals, np.zeros(pad.size, np.uint64)])
    N = keys.size
    if is_tight or before is None:
        a, b = n, N
    else:  # (never before the restore: the image inserts are in the image)
        a, b = max(n, 2 * n - before), min(N, 2 * n + 1 + after)
    step = min(max(b - a, 64), max_batch)
    bounds = sorted(set(range(n, a, 256)) | {a, b, N} | set(range(b, N, step)))
    with knobs(TIGHT if is_tight else {}):
        t = P.CCEH(init_cap, convention=conv, max_batch=max_batch, max_segments=64)
    t.restore(img)
    t.timing(events=True)
    out = np.zeros(N, np.uint64)
    st = np.zeros(N, np.uint8)
    st[:n] = st_img
    took = None
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        _classes(t)
        out[lo:hi], st[lo:hi] = t.Mixed(ops[lo:hi], keys[lo:hi], vals[lo:hi])
        if lo <= 2 * n < hi:
            took = _kernel(_classes(t), hi - lo)
    assert took == kernel, (took, kernel)
    ov, ost, od, loss = serial[name]
    m = ov.size
    assert np.all(out[m:] == 0) and np.all(st[m:] == P.ST_MISS)
    want = S.split_shape_get_values(golden[name], ops[:m], keys[:m], vals[:m])
    _check_ops(out[:m], st[:m], ops[:m], golden[name], ov, ost, want)
    _check_table(t, golden[name], od, loss)  # (B's own counters: the drops all happen after the restore)
    assert snap(t) == I.image_from_dump(od, t.initial_depth)
    t.close()


@pytest.mark.parametrize("batch,max_batch", [(1, 4096), (64, 4096), (256, 4096), (500, 500), (0, 8192), (0, 1 << 14)])
def test_split_loss_mixed_cut_before_its_trigger(batch, max_batch, scen):
    """A takes split_loss_mixed up to its first trigger (the windows are full,
    nothing has split); B, restored, takes the rest: the splits, their drops
    and the Gets around them."""
    init_cap, conv, ops, keys, vals = scen["split_loss_mixed"]
    cut = 32 + 28 + 32 + 28
    assert ops[cut] == S.OP_INSERT and np.all(ops[cut - 60:cut] == S.OP_GET)
    o = O.OracleCCEH(1)
    ov, ost = o.mixed(ops, keys, vals)
    a = P.CCEH(init_cap, max_batch=4096, max_segments=256)
    out_a, st_a = run(a, ops[:cut], keys[:cut], vals[:cut], 64)
    assert a.stats()["splits"] == 0
    b = P.CCEH(init_cap, max_batch=max_batch, max_segments=256)
    b.restore(a.snapshot())
    out_b, st_b = run(b, ops[cut:], keys[cut:], vals[cut:], batch or len(ops))
    same_answers(np.concatenate([out_a, out_b]), np.concatenate([st_a, st_b]), ov, ost)
    same_dump(b.dump(), o.dump())
    s = b.stats()
    assert s["split_loss"] == o.stats()["split_loss"] > 0 and s["error_flags"] == 0
    a.close()
    b.close()


@pytest.mark.parametrize("name,max_batch", [("mixed_cap2_30k_ins80", 4096), ("cap2_ins100k", 1 << 14)])
def test_restore_while_ramping_then_rebucket(name, max_batch, scen):
    """Cut at a third (of the stream; of cap2_ins100k's inserts), where the
    directory still has fewer bucket bits than p1max: the restored engine
    starts at min(p1max, min local depth) bits and later rebuckets the
    directory the restore built."""
    init_cap, conv, ops, keys, vals = scen[name]
    if name == "cap2_ins100k":  # its Gets follow its 100k inserts: keep 20k of them
        n_ins = int((ops == S.OP_INSERT).sum())
        ops, keys, vals = ops[:n_ins + 20000], keys[:n_ins + 20000], vals[:n_ins + 20000]
        cut = n_ins // 3
    else:
        cut = len(ops) // 3
    p1max = max_batch.bit_length() - 1 - 7
    o = O.OracleCCEH(1)
    ov, ost = o.mixed(ops[:cut], keys[:cut], vals[:cut])
    min_ld = int(o.dump()["local_depth"].min())
    assert min_ld < p1max  # the premise: still ramping at the cut
    a = P.CCEH(init_cap, max_batch=max_batch, max_segments=1024)
    out_a, st_a = run(a, ops[:cut], keys[:cut], vals[:cut], max_batch)
    same_answers(out_a, st_a, ov, ost)
    img = snap(a)
    assert img == I.image_from_dump(o.dump(), 1)
    b = P.CCEH(init_cap, max_batch=max_batch, max_segments=1024)
    b.restore(img)
    assert b.stats()["bucket_bits"] == min(p1max, min_ld)
    out_b, st_b = run(b, ops[cut:], keys[cut:], vals[cut:], max_batch)
    ov, ost = o.mixed(ops[cut:], keys[cut:], vals[cut:])
    same_answers(out_b, st_b, ov, ost)
    same_dump(b.dump(), o.dump())
    s = b.stats()
    assert s["bucket_bits"] == p1max and s["error_flags"] == 0
    assert snap(b) == I.image_from_dump(o.dump(), 1)
    a.close()
    b.close()


# ---- 4. across geometries

# id -> (scenario, ops before the cut, the target's max_batch, knobs, how its sub-directories must be placed)
GEOMETRIES = {
    "p1max1_fixed_slots_db_le_7": ("mixed_cap2_30k_ins80", 15000, 500, {}, "fixed"),
    "p1max1_pool_db_gt_7": ("cap256_ins400k", 200000, 500, {}, "pool"),
    "p1max7_ramping_pool": ("mixed_cap2_30k_ins80", 15000, 1 << 14, {}, "ramp"),
    "tight_fixed_slots": ("mixed_cap2_30k_ins80", 15000, 4096, TIGHT, "fixed"),
}


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_restore_across_geometries(geo, scen):
    """Snapshot from max_batch = 4096 (p1max 5), restore into engines whose
    directory has another shape: p1 == p1max with every sub-directory in its
    fixed slot (at most 2^7 entries), with sub-directories past 2^7 entries
    in the pool, and with p1 < p1max."""
    name, cut, max_batch, env, place = GEOMETRIES[geo]
    init_cap, conv, ops, keys, vals = scen[name]
    if name == "cap256_ins400k":  # 400k inserts, then Gets: 300k inserts and 20k of the Gets
        ops, keys, vals = (np.concatenate([x[:300000], x[400000:420000]]) for x in (ops, keys, vals))
    d0 = _depth(init_cap, conv)
    o = O.OracleCCEH(d0)
    ov, ost = o.mixed(ops[:cut], keys[:cut], vals[:cut])
    a = P.CCEH(init_cap, convention=conv, max_batch=4096, max_segments=2048)
    a.MixedBatches(ops[:cut], keys[:cut], vals[:cut], list(range(0, cut, 4096)) + [cut])
    img = snap(a)
    a.close()
    assert img == I.image_from_dump(o.dump(), d0)
    ld = o.dump()["local_depth"]
    with knobs(env):
        b = P.CCEH(init_cap, convention=conv, max_batch=max_batch, max_segments=2048)
    b.restore(img)
    p1max = 1 if env or max_batch == 500 else max_batch.bit_length() - 1 - 7
    p1 = b.stats()["bucket_bits"]
    assert p1 == min(p1max, int(ld.min()))
    if place == "fixed":    # p1 == p1max and db <= 7
        assert p1 == p1max and int(ld.max()) - p1 <= 7
    elif place == "pool":   # p1 == p1max and db > 7
        assert p1 == p1max and int(ld.max()) - p1 > 7
    else:
        assert p1 < p1max
    same_dump(b.dump(), o.dump())
    n = len(ops)
    out, st = b.MixedBatches(ops[cut:], keys[cut:], vals[cut:],
                             [i - cut for i in range(cut, n, max_batch)] + [n - cut])
    ov, ost = o.mixed(ops[cut:], keys[cut:], vals[cut:])
    same_answers(out, st, ov, ost)
    same_dump(b.dump(), o.dump())
    assert b.stats()["error_flags"] == 0 and b.stats()["splits"] > 0
    b.close()


def test_restore_into_upsert_engine():
    """The upsert flag is no part of the table: an image written by an upsert
    engine restores into both kinds, and the upsert one continues an
    upsert_scenarios stream like OracleCCEH(upsert=True)."""
    init_cap, conv, ops, keys, vals = S.upsert_scenarios(O.hash64)["up_reinserts_cap2"]
    cut = len(ops) // 2
    o = O.OracleCCEH(1, upsert=True)
    o.mixed(ops[:cut], keys[:cut], vals[:cut])
    a = P.CCEH(init_cap, max_batch=4096, max_segments=512, upsert=True)
    run(a, ops[:cut], keys[:cut], vals[:cut], 4096)
    img = snap(a)
    assert img == I.image_from_dump(o.dump(), 1)
    plain = P.CCEH(init_cap, max_batch=4096, max_segments=512)
    plain.restore(img)
    same_dump(plain.dump(), o.dump())
    plain.close()
    b = P.CCEH(init_cap, max_batch=1 << 14, max_segments=512, upsert=True)
    b.restore(a.snapshot())
    out, st = run(b, ops[cut:], keys[cut:], vals[cut:], 1 << 14)
    ov, ost = o.mixed(ops[cut:], keys[cut:], vals[cut:])
    same_answers(out, st, ov, ost)
    assert np.any(st == P.ST_UPDATED)
    same_dump(b.dump(), o.dump())
    a.close()
    b.close()


# ---- 5. sharded

def test_sharded_round_trip_and_refusals(scen):
    """shard_bits = 2: every shard snapshots at the half, is restored into a
    new engine and continues; the four restored shards reassemble the global
    serial table.  An image restores only into its own shard and initial depth."""
    init_cap, conv, ops, keys, vals = scen["cap8_ins20k"]
    ops, keys, vals = ops[:25000], keys[:25000], vals[:25000]
    owner = (P.hash64(keys) >> np.uint64(62)).astype(np.int64)
    o = O.OracleCCEH(3)
    o.mixed(ops, keys, vals)
    od = o.dump()
    seg_owner = (od["prefix"] >> (od["local_depth"].astype(np.uint64) - np.uint64(2))).astype(np.int64)
    parts, images = [], []
    for sh in range(4):
        sel = np.nonzero(owner == sh)[0]
        half = sel.size // 2
        a = P.CCEH(depth=3, shard_bits=2, shard_id=sh, max_batch=4096, max_segments=256)
        run(a, ops[sel[:half]], keys[sel[:half]], vals[sel[:half]], 4096)
        img = snap(a)
        h = I.validate(img)
        assert (h["shard_bits"], h["shard_id"], h["initial_depth"]) == (2, sh, 3)
        b = P.CCEH(depth=3, shard_bits=2, shard_id=sh, max_batch=1 << 13, max_segments=256)
        b.restore(img)
        same_dump(b.dump(), a.dump())
        assert snap(b) == img
        a.close()
        run(b, ops[sel[half:]], keys[sel[half:]], vals[sel[half:]], 1 << 13)
        d = b.dump()
        parts.append(d)
        # the shard's image is the global table's segments of its prefix
        mine = seg_owner == sh
        slots = np.repeat(mine, 1024)
        sub = {"local_depth": od["local_depth"][mine], "keys": od["keys"][slots], "values": od["values"][slots]}
        images.append(snap(b))
        assert images[-1] == I.image_from_dump(sub, 3, shard_bits=2, shard_id=sh)
        assert np.array_equal(d["prefix"], od["prefix"][mine])
        assert b.stats()["error_flags"] == 0
        b.close()
    for f in ("keys", "values", "local_depth"):
        assert np.array_equal(np.concatenate([d[f] for d in parts]), od[f]), f
    # another shard, another initial depth: refused, the target untouched
    for kw in (dict(depth=3, shard_bits=2, shard_id=1), dict(depth=4, shard_bits=2, shard_id=0),
               dict(depth=3, shard_bits=0, shard_id=0)):
        t = P.CCEH(max_batch=4096, max_segments=256, **kw)
        mine = uniform_keys(5, 0, 4000)
        t.Insert(mine, mine)
        before = t.dump()
        with pytest.raises(P.PmdfcError) as e:
            t.restore(images[0])
        assert code(e) == ERR_ARG
        same_dump(t.dump(), before)
        t.close()


# ---- 6. over a used table

def test_restore_over_a_larger_used_table(scen, finals):
    """The target first grows deeper and into more segments than the image
    holds: nothing of it may survive the restore."""
    init_cap, conv, ops, keys, vals = scen["cap2_ins3k"]
    d0, o, od, img = finals["cap2_ins3k"]
    t = P.CCEH(init_cap, max_batch=1 << 16, max_segments=1024)
    old = uniform_keys(31337, 0, 50000)
    assert np.all(t.Insert(old, old) == P.ST_INSERTED)
    s = t.stats()
    assert s["segments"] > 4 * len(od["local_depth"]) and s["depth"] > od["depth"]
    t.restore(img)
    same_dump(t.dump(), od)
    gv, gs = t.Get(old)
    assert np.all(gs == P.ST_MISS) and not gv.any()
    s = t.stats()
    assert s["segments"] == len(od["local_depth"]) and s["depth"] == od["depth"] and s["splits"] == 0
    assert abs(t.Utilization() - o.utilization()) < 1e-9
    assert snap(t) == img
    o2 = O.OracleCCEH(d0)
    o2.mixed(ops, keys, vals)
    more = uniform_keys(31338, 0, 20000)
    st = np.concatenate([t.Insert(more[lo:lo + 5000], more[lo:lo + 5000] ^ np.uint64(3)) for lo in range(0, 20000, 5000)])
    assert np.array_equal(st, o2.insert(more, more ^ np.uint64(3)))
    same_dump(t.dump(), o2.dump())
    q = np.concatenate([keys, more, old[:2000]])
    gv, gs = t.Get(q)
    ov, os_ = o2.get(q)
    same_answers(gv, gs, ov, os_)
    assert t.stats()["error_flags"] == 0
    t.close()


# ---- 7. refusals

def _used_engine(**kw):
    t = P.CCEH(8, max_batch=4096, **kw)
    k = uniform_keys(99, 0, 6000)
    t.Insert(k, k)
    return t, t.dump()


def test_snapshot_buffer_one_byte_short(finals):
    t = P.CCEH(2, max_batch=4096, max_segments=64)
    t.restore(finals["cap2_ins3k"][3])
    L = P.load_library()
    need = C.c_uint64()
    assert L.pmdfc_cceh_snapshot(t.handle, None, 0, C.byref(need), None) == ERR_SIZE
    assert need.value == len(finals["cap2_ins3k"][3])
    buf = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    got = C.c_uint64()
    assert L.pmdfc_cceh_snapshot(t.handle, buf.data_ptr(), need.value - 1, C.byref(got), None) == ERR_SIZE
    assert got.value == need.value and not buf.any()  # the exact size, nothing written
    assert L.pmdfc_cceh_snapshot(t.handle, buf.data_ptr(), need.value, C.byref(got), None) == 0
    assert buf.cpu().numpy().tobytes() == finals["cap2_ins3k"][3]
    t.close()


def test_restore_refuses_more_segments_than_the_arena(finals):
    d0, o, od, img = finals["cap8_ins20k"]
    nseg = len(od["local_depth"])
    t, before = _used_engine(max_segments=nseg - 1)
    assert t.stats()["max_segments"] == nseg - 1
    with pytest.raises(P.PmdfcError) as e:
        t.restore(img)
    assert code(e) == ERR_SIZE
    same_dump(t.dump(), before)
    t.close()
    t, _ = _used_engine(max_segments=nseg)
    t.restore(img)
    same_dump(t.dump(), od)
    t.close()


def test_restore_refuses_corrupt_headers_and_depths(finals):
    """Each corruption of the CPU test: refused on the host, so no kernel ran
    on the image and the table is as before."""
    d0, o, od, img = finals["cap8_ins20k"]
    t, before = _used_engine(max_segments=256)
    bad = corruptions(img, d0)
    assert len(bad) == 7
    for case, b in bad.items():
        with pytest.raises(P.PmdfcError) as e:
            t.restore(b)
        assert code(e) == ERR_ARG, case
        same_dump(t.dump(), before)
    assert t.stats()["splits"] > 0  # not even the counters were touched
    t.restore(img)
    same_dump(t.dump(), od)
    t.close()


def test_restore_refuses_keys_outside_their_segment(finals):
    """Two live keys exchanged between two segments of different prefix pass
    every host check; the device pass counts them, and the table is left
    freshly reset.  So does a reserved key."""
    d0, o, od, img = finals["cap8_ins20k"]
    a = np.frombuffer(img, np.uint8).copy()
    nseg = len(od["local_depth"])
    pairs = a[I.HEADER_BYTES + I.depth_bytes(nseg):].view(np.uint64).reshape(nseg, 1024, 2)
    live = pairs[:, :, 0] != np.uint64(2**64 - 1)
    s0, s1 = 0, nseg - 1
    assert od["prefix"][s0] != od["prefix"][s1] or od["local_depth"][s0] != od["local_depth"][s1]
    i0, i1 = int(np.nonzero(live[s0])[0][0]), int(np.nonzero(live[s1])[0][0])
    swapped = a.copy()
    sp = swapped[I.HEADER_BYTES + I.depth_bytes(nseg):].view(np.uint64).reshape(nseg, 1024, 2)
    sp[s0, i0], sp[s1, i1] = pairs[s1, i1].copy(), pairs[s0, i0].copy()
    I.validate(swapped)  # nothing the host can see
    sentinel = a.copy()
    sentinel[I.HEADER_BYTES + I.depth_bytes(nseg):].view(np.uint64).reshape(nseg, 1024, 2)[s0, i0, 0] = 2**64 - 2
    fresh = P.CCEH(8, max_batch=4096, max_segments=256)
    want = fresh.dump()
    fresh.close()
    for b in (swapped, sentinel):
        t, _ = _used_engine(max_segments=256)
        with pytest.raises(P.PmdfcError) as e:
            t.restore(b)
        assert code(e) == ERR_ARG
        same_dump(t.dump(), want)
        s = t.stats()
        assert s["segments"] == 8 and s["splits"] == 0 and s["error_flags"] == 0
        k = uniform_keys(98, 0, 3000)  # and it works on from there
        o2 = O.OracleCCEH(3)
        assert np.array_equal(t.Insert(k, k), o2.insert(k, k))
        same_dump(t.dump(), o2.dump())
        t.close()


# ---- 8. front-end and files

def _ring_order(pl):
    return np.argsort(pl, kind="stable")  # ring-major (ring = place >> 48), place order within a ring


@pytest.mark.parametrize("waves", [1, 8])
def test_kv_save_load_through_the_rings(waves, scen, tmp_path):
    init_cap, conv, ops, keys, vals = scen["mixed_cap2_30k_ins80"]
    half = len(ops) // 2
    path = tmp_path / "table.img"
    o = O.OracleCCEH(1)
    kv = KV(init_cap, max_batch=4096, max_segments=1024, serve_waves=waves)
    vo, st, pl = kv.ops(ops[:half], keys[:half], vals[:half], run=0)
    order = _ring_order(pl)
    ov, ost = o.mixed(ops[:half][order], keys[:half][order], vals[:half][order])
    same_answers(vo[order], st[order], ov, ost)
    kv.save(path)
    assert path.read_bytes() == I.image_from_dump(o.dump(), 1)
    assert kv.phase()["failed_ops"] == 0
    kv.close()
    kv = KV(init_cap, max_batch=4096, max_segments=1024, serve_waves=waves)
    kv.load(path)
    same_dump(kv.dump(), o.dump())
    vo, st, pl = kv.ops(ops[half:], keys[half:], vals[half:], run=0)
    order = _ring_order(pl)
    ov, ost = o.mixed(ops[half:][order], keys[half:][order], vals[half:][order])
    same_answers(vo[order], st[order], ov, ost)
    same_dump(kv.dump(), o.dump())
    ph = kv.phase()
    assert ph["failed_ops"] == 0 and ph["serve_waves"] == min(waves, 2)
    assert kv.stats()["error_flags"] == 0
    with pytest.raises(P.PmdfcError):
        kv.load(tmp_path / "missing.img")
    same_dump(kv.dump(), o.dump())
    kv.close()


def test_cceh_save_load_file(finals, tmp_path):
    d0, o, od, img = finals["dup_wrap"]
    t = P.CCEH(depth=d0, max_batch=4096, max_segments=256)
    t.restore(np.frombuffer(img, np.uint8))  # (a numpy array; bytes and tensors elsewhere)
    path = tmp_path / "t.img"
    assert t.save(path) == len(img)
    assert path.read_bytes() == snap(t) == img
    u = P.CCEH(depth=d0, max_batch=500, max_segments=256)
    u.load(path)
    same_dump(u.dump(), od)
    kv = KV(depth=d0, max_batch=4096, max_segments=256, serve_waves=1)  # and the front-end reads the same file
    kv.load(path)
    same_dump(kv.dump(), od)
    kv.close()
    t.close()
    u.close()


def test_facades_save_and_load(tmp_path):
    """GpuCCEH : IHash and GpuCCEHHybrid : ICCEH (tests/cpp/test_gpu_image_kv.cpp,
    a program of its own: the facades are C++): a saved table loaded by a new
    backend object answers every Get and takes more inserts, either facade
    reads the other's file, refused files leave the table alone, and Save /
    Load from a completion callback fail at once."""
    exe = os.path.join(os.path.dirname(P.engine.LIB_PATH), "test_gpu_image_kv")
    r = subprocess.run([exe, str(tmp_path), "6000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("GpuCCEH round_trip_bad 0", "GpuCCEHHybrid round_trip_bad 0", "cross_load_bad 0", "callback_bad 0",
                 "image_kv_bad 0"):
        assert line in r.stdout, r.stdout
